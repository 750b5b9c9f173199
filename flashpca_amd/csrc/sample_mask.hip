// sample_mask.hip -- sample subsets: fpca_set_sample_mask / fpca_nkept (include/fpca.h "Sample subset").
//
// PCs are fitted on a subset of the samples and everyone else is projected onto them.  The packed matrix stays where it is; what a
// subset changes is the standardisation (three small arrays) and which rows of the operator's blocks may be non-zero:
//   k_bed_stats_masked  ONE pass over the packed stream, one workgroup per SNP: the kept-sample counts of dosage 0 / 1 / 2 are popcounts
//                       of K1's bit planes under one mask row in the packed layout (shared by all workgroups, so it is served out of L2);
//                       mean / sd / table / sum of squares follow by K1's formulas in K1's order (k_bed_stats; data.cpp:266-291), which
//                       makes them bit-identical to K1 on the re-packed subset.  The missing-call count is that of ALL N samples: the
//                       route cost model and the gather lists describe the packed matrix, which does not change.
//   k_mask_rows         zeroes the held-out rows of a row-major [N_pad][b] block (stores only; kept rows are not touched).  K2 on a block
//                       whose held-out rows are zero is X_kept' B_kept, K3 computes every row, so masking its result gives X_kept X_kept' B.
//   k_gather_kept / k_scatter_kept   the kept rows of a block <-> column-major n_kept x ncols: the eigensolver sees a problem of n_kept
//                       rows (its divisor, its dimension limit and its small-N route follow from that alone).
// Kernel boundaries are the only synchronisation between workgroups; no atomics, so a repeat call is bit-identical.
#include <algorithm>
#include <cmath>

#include "ctx.hpp"

using namespace fpca;

namespace {

// the kept samples' dosage counts and all samples' missing count of one 32-bit word (16 samples); m has bit 2 s set for kept sample s
__device__ __forceinline__ void count_word_masked(uint32_t w, uint32_t m, uint32_t &k00, uint32_t &k10, uint32_t &k11, uint32_t &c01)
{
   const uint32_t lo = w & 0x55555555u, hi = (w >> 1) & 0x55555555u;
   k11 += __popc(lo & hi & m);
   k10 += __popc(hi & ~lo & m);
   k00 += __popc(~(lo | hi) & m);
   c01 += __popc(lo & ~hi);
}

__global__ __launch_bounds__(256) void k_bed_stats_masked(const uint8_t *__restrict__ packed, size_t pitch, const uint8_t *__restrict__ keep_bits,
                                                           uint64_t N, int stand_method, double *__restrict__ lut, double *__restrict__ mean_out,
                                                           double *__restrict__ sd_out, double *__restrict__ sumsq_out,
                                                           uint32_t *__restrict__ nmiss_out)
{
   const uint64_t snp = blockIdx.x;
   const uint4 *row = reinterpret_cast<const uint4 *>(packed + snp * pitch);
   const uint4 *mrow = reinterpret_cast<const uint4 *>(keep_bits);
   const uint32_t nvec = (uint32_t)(pitch / 16);
   uint32_t k00 = 0, k10 = 0, k11 = 0, c01 = 0;
   for (uint32_t v = threadIdx.x; v < nvec; v += 256) {
      const uint4 q = row[v], m = mrow[v];
      count_word_masked(q.x, m.x, k00, k10, k11, c01);
      count_word_masked(q.y, m.y, k00, k10, k11, c01);
      count_word_masked(q.z, m.z, k00, k10, k11, c01);
      count_word_masked(q.w, m.w, k00, k10, k11, c01);
   }
   for (int off = 32; off > 0; off >>= 1) {
      k00 += __shfl_down(k00, off);
      k10 += __shfl_down(k10, off);
      k11 += __shfl_down(k11, off);
      c01 += __shfl_down(c01, off);
   }
   __shared__ uint32_t red[4][4];
   const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
   if (lane == 0) {
      red[wave][0] = k00;
      red[wave][1] = k10;
      red[wave][2] = k11;
      red[wave][3] = c01;
   }
   __syncthreads();
   if (threadIdx.x == 0) {
      uint64_t n00 = 0, n10 = 0, n11 = 0, n01 = 0;
      for (int w = 0; w < 4; w++) {
         n00 += red[w][0];
         n10 += red[w][1];
         n11 += red[w][2];
         n01 += red[w][3];
      }
      const uint64_t ngood = n00 + n10 + n11;
      // data.cpp:266-275 on the kept samples (an all-missing SNP: 0 / 0, as in K1)
      const double mean = (double)(2 * n00 + n10) / (double)ngood;
      const double pp = mean / 2.0;
      double sd;
      if (stand_method == 2)
         sd = sqrt(pp * (1 - pp)); // STANDARDISE_BINOM  (data.cpp:279)
      else
         sd = sqrt(2.0 * pp * (1 - pp)); // STANDARDISE_BINOM2 (data.cpp:281)
      // data.cpp:299-320: table indexed by RAW code; all-zero when sd <= VAR_TOL (or NaN) -- a SNP monomorphic among the kept samples
      // is a zero column
      double v0 = 0, v2 = 0, v3 = 0;
      if (sd > 1e-9) {
         v3 = (0.0 - mean) / sd;
         v2 = (1.0 - mean) / sd;
         v0 = (2.0 - mean) / sd;
      }
      double *lp = lut + snp * 4;
      lp[0] = v0;
      lp[1] = 0.0;
      lp[2] = v2;
      lp[3] = v3;
      mean_out[snp] = mean;
      sd_out[snp] = sd;
      nmiss_out[snp] = (uint32_t)(n01 - ((uint64_t)pitch * 4 - N)); // missing calls among ALL N samples (padding is "01" too)
      sumsq_out[snp] = (double)n00 * v0 * v0 + (double)n10 * v2 * v2 + (double)n11 * v3 * v3;
   }
}

// blk: row-major [rows][b], b a multiple of 2; one thread per pair of columns, stores to the held-out rows only
__global__ __launch_bounds__(256) void k_mask_rows(double *__restrict__ blk, uint64_t rows, int half_b, const uint8_t *__restrict__ keep)
{
   const uint64_t total = rows * (uint64_t)half_b;
   double2 *p = reinterpret_cast<double2 *>(blk);
   for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (uint64_t)gridDim.x * 256)
      if (!keep[i / (uint64_t)half_b]) p[i] = make_double2(0.0, 0.0);
}

__global__ void k_gather_kept(const double *__restrict__ blk, int b, int ncols, const uint32_t *__restrict__ idx, uint64_t nk, double *__restrict__ out)
{
   const uint64_t total = nk * ncols;
   for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (uint64_t)gridDim.x * 256) {
      const uint64_t r = i / ncols;
      const int c = (int)(i % ncols);
      out[(uint64_t)c * nk + r] = blk[(uint64_t)idx[r] * b + c];
   }
}

// (the block has been zeroed: the held-out rows, the pad rows and the columns >= ncols stay zero)
__global__ void k_scatter_kept(const double *__restrict__ in, int b, int ncols, const uint32_t *__restrict__ idx, uint64_t nk, double *__restrict__ blk)
{
   const uint64_t total = nk * ncols;
   for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (uint64_t)gridDim.x * 256) {
      const uint64_t r = i / ncols;
      const int c = (int)(i % ncols);
      blk[(uint64_t)idx[r] * b + c] = in[(uint64_t)c * nk + r];
   }
}

unsigned grid_for(uint64_t total) { return (unsigned)std::min<uint64_t>(8192, std::max<uint64_t>(1, (total + 255) / 256)); }

void free_mask(fpca_ctx *c)
{
   if (c->d_keep) (void)hipFree(c->d_keep);
   if (c->d_keep_bits) (void)hipFree(c->d_keep_bits);
   if (c->d_keep_idx) (void)hipFree(c->d_keep_idx);
   c->d_keep = c->d_keep_bits = nullptr;
   c->d_keep_idx = nullptr;
   c->h_keep_idx.clear();
   c->n_kept = 0;
}

} // namespace

namespace fpca {

void masked_stats(fpca_ctx *c)
{
   std::vector<uint32_t> nm(c->P_g);
   std::vector<double> ss(c->P_g);
   if (c->P_g) {
      DevMem<uint32_t> d_nmiss(c->P_g, "fpca_set_sample_mask", "the per-SNP missing counts");
      hipLaunchKernelGGL(k_bed_stats_masked, dim3((unsigned)c->P_g), dim3(256), 0, c->stream, c->d_packed, c->pitch, c->d_keep_bits, c->N, c->stand,
                         c->d_lut, c->d_mean, c->d_sd, c->d_sumsq, d_nmiss.p);
      const hipError_t e[3] = {hipGetLastError(), hipMemcpyAsync(ss.data(), c->d_sumsq, c->P_g * sizeof(double), hipMemcpyDeviceToHost, c->stream),
                               hipMemcpyAsync(nm.data(), d_nmiss.p, c->P_g * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream)};
      const hipError_t es = hipStreamSynchronize(c->stream); // (before anything is reported: d_nmiss is freed on the way out)
      for (hipError_t x : e) HIP_CHECK(x);
      HIP_CHECK(es);
   }
   c->n_missing = 0;
   for (uint32_t v : nm) c->n_missing += v;
   c->missing_known = true;
   c->h_nmiss.swap(nm);
   c->trace_local = blocked_sum(ss.data(), ss.size()); // (as ensure_stats)
   c->i8_scales_done = false;
   c->stats_done = true;
}

void mask_rows(const fpca_ctx *c, double *blk, int b, hipStream_t s)
{
   hipLaunchKernelGGL(k_mask_rows, dim3(grid_for(c->N_pad * (uint64_t)(b / 2))), dim3(256), 0, s, blk, c->N_pad, b / 2, c->d_keep);
   HIP_CHECK(hipGetLastError());
}

void gather_kept(const fpca_ctx *c, const double *blk, int b, int ncols, double *out, hipStream_t s)
{
   hipLaunchKernelGGL(k_gather_kept, dim3(grid_for(c->n_kept * (uint64_t)ncols)), dim3(256), 0, s, blk, b, ncols, c->d_keep_idx, c->n_kept, out);
   HIP_CHECK(hipGetLastError());
}

void scatter_kept(const fpca_ctx *c, const double *in, int b, int ncols, double *blk, hipStream_t s)
{
   HIP_CHECK(hipMemsetAsync(blk, 0, (size_t)c->N_pad * b * sizeof(double), s));
   hipLaunchKernelGGL(k_scatter_kept, dim3(grid_for(c->n_kept * (uint64_t)ncols)), dim3(256), 0, s, in, b, ncols, c->d_keep_idx, c->n_kept, blk);
   HIP_CHECK(hipGetLastError());
}

void refuse_masked(const fpca_ctx *c, const char *fn)
{
   if (c && c->masked())
      throw Error(FPCA_EINVAL, std::string(fn) + ": a sample mask is set (fpca_set_sample_mask); sample subsets apply to fpca_stats, the operator and "
                                                 "fpca_pca only -- clear the mask first");
}

void refuse_shard_while_masked(const fpca_ctx *c, const char *fn)
{
   if (c && c->masked())
      throw Error(FPCA_EINVAL, std::string(fn) + ": a sample mask is set (fpca_set_sample_mask); sample subsets run on a single context only, "
                                                 "not on one shard of several -- clear the mask first");
}

} // namespace fpca

extern "C" int fpca_set_sample_mask(fpca_ctx *ctx, const uint8_t *keep)
{
   return guarded([&] {
      if (!ctx) throw Error(FPCA_EINVAL, "bad argument to fpca_set_sample_mask (NULL context)");
      if (!keep) { // back to all N samples: K1 runs again at the next use, as on a fresh context
         if (!ctx->masked()) return;
         HIP_CHECK(hipSetDevice(ctx->device));
         HIP_CHECK(hipStreamSynchronize(ctx->stream));
         free_mask(ctx);
         ctx->stats_done = false;
         ctx->trace_local = 0;
         ctx->i8_scales_done = false;
         return;
      }
      if (ctx->dense)
         throw Error(FPCA_EINVAL, "fpca_set_sample_mask: this context holds a dense matrix, of which only the standardised copy is kept; re-standardising "
                                  "on a subset needs the packed genotypes (fpca_create, fpca_create_from_bed, synthetic)");
      if (ctx->multi() || (ctx->rank_known && ctx->nranks > 1))
         throw Error(FPCA_EINVAL, "fpca_set_sample_mask: the context is one shard of several (a communicator, an all-reduce hook or fpca_set_rank with "
                                  "more than one rank); sample subsets run on a single context only");
      if (ctx->meansd_preloaded)
         throw Error(FPCA_EINVAL, "fpca_set_sample_mask: this context carries a preloaded mean/sd (fpca_set_meansd); a sample mask would replace it with "
                                  "the statistics of the kept samples");
      const uint64_t N = ctx->N;
      std::vector<uint32_t> idx;
      std::vector<uint8_t> rows(ctx->N_pad, 0), bits(ctx->pitch, 0);
      for (uint64_t i = 0; i < N; i++)
         if (keep[i]) {
            idx.push_back((uint32_t)i);
            rows[i] = 1;
            bits[i / 4] |= (uint8_t)(1u << (2 * (i % 4)));
         }
      if (idx.size() < 2)
         throw Error(FPCA_EINVAL, "fpca_set_sample_mask: the mask keeps " + std::to_string(idx.size()) + " of " + std::to_string(N) +
                                     " samples; at least 2 are needed");
      HIP_CHECK(hipSetDevice(ctx->device));
      HIP_CHECK(hipStreamSynchronize(ctx->stream));
      static const char *FN = "fpca_set_sample_mask";
      DevMem<uint8_t> d_rows(rows.size(), FN, "the row mask"), d_bits(bits.size(), FN, "the mask row of the statistics pass");
      DevMem<uint32_t> d_idx(idx.size(), FN, "the kept-sample list");
      HIP_CHECK(hipMemcpy(d_rows.p, rows.data(), rows.size(), hipMemcpyHostToDevice));
      HIP_CHECK(hipMemcpy(d_bits.p, bits.data(), bits.size(), hipMemcpyHostToDevice));
      HIP_CHECK(hipMemcpy(d_idx.p, idx.data(), idx.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
      free_mask(ctx); // all three uploads are in: the context takes them
      ctx->d_keep = d_rows.release();
      ctx->d_keep_bits = d_bits.release();
      ctx->d_keep_idx = d_idx.release();
      ctx->n_kept = idx.size();
      ctx->h_keep_idx.swap(idx);
      ctx->stats_done = false;
      ctx->trace_local = 0;
      ctx->i8_scales_done = false;
      ensure_stats(ctx); // the one pass: kept-sample statistics and the all-sample missing counts
   });
}

extern "C" uint64_t fpca_nkept(const fpca_ctx *ctx) { return ctx ? (ctx->masked() ? ctx->n_kept : ctx->N) : 0; }
