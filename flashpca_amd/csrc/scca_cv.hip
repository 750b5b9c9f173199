// scca_cv.hip -- K-fold cross-validation of the SCCA penalties (the R function cv.scca(), flashpcaR/R/scca.R:410-557): fpca_scca_cv and
// the hook fpca_debug_fold_stats.
//
// The reference refits scca(X[w,], Y[w,]) per fold on a numeric matrix.  Here the packed matrix stays where it is:
//   k_fold_counts    ONE pass over the packed stream gives, per SNP and fold, the held-out counts of dosage 0 / 1 / 2: popcounts of K1's
//                    even / odd bit planes under per-fold sample masks in the packed layout.  Integers, hence exact.
//   k_fold_meansd    training counts = total - the fold's own -> mean, sd by K1's formulas in K1's order (bit-identical to K1 on the
//                    re-packed training rows); the context's d_mean / d_sd / d_lut are swapped per fold and restored by a guard.
//   k_cv_stand_y     the phenotypes standardised on the training rows (k_dense_standardise's rules under a row mask), all N rows out
//   k_cv_operand     K2's operand: the standardised phenotypes * invdiv with the held-out rows ZERO, so xt_dev gives X_train' Y_train
//   scca_fit_dev     (scca.hip) n1 n2 + 1 fits per fold on the resident C_f; U and V of every model stay on the device
//   k_cv_count_nz    non-zeros of every column of the fold's U
//   x_dev + k_cv_gather_x   K3 computes EVERY row of X U; the held-out rows are the predictions, copied into the resident xpred
//   k_cv_ypred       the held-out rows of Y V
//   k_cv_corr        pooled Pearson correlation of every column pair: two passes (means, then centred sums), partial sums added in a
//                    fixed order -- a repeat run is bit-identical
// Everything runs on the context's stream; kernel boundaries are the only synchronisation between workgroups.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <limits>
#include <memory>

#include "../../include/fpca_debug.h"
#include "ctx.hpp"
#include "scca.hpp"

using namespace fpca;

namespace {

constexpr int FG = 8; // folds counted per sweep over a SNP's record: 24 counters per thread; the later sweeps re-read the record from L2

// counts[f][snp][0..2] = held-out samples of fold f with dosage 0, 1, 2 (raw codes 11, 10, 00).  One workgroup per SNP; masks[f] is a
// pitch-byte row with bit 2 (i % 4) of byte i / 4 set for the samples i of fold f and nothing on the pad samples.
__global__ __launch_bounds__(256) void k_fold_counts(const uint8_t *__restrict__ packed, size_t pitch, const uint8_t *__restrict__ masks,
                                                     int nfolds, uint64_t P_g, uint32_t *__restrict__ counts)
{
   const uint64_t snp = blockIdx.x;
   const uint4 *row = reinterpret_cast<const uint4 *>(packed + snp * pitch);
   const uint32_t nvec = (uint32_t)(pitch / 16);
   __shared__ uint32_t red[4][FG * 3];
   const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
   for (int f0 = 0; f0 < nfolds; f0 += FG) {
      uint32_t c[FG][3];
#pragma unroll
      for (int g = 0; g < FG; g++) c[g][0] = c[g][1] = c[g][2] = 0;
      for (uint32_t v = threadIdx.x; v < nvec; v += 256) {
         const uint4 q = row[v];
         const uint32_t w[4] = {q.x, q.y, q.z, q.w};
         uint32_t p11[4], p10[4], p00[4];
#pragma unroll
         for (int i = 0; i < 4; i++) {
            const uint32_t lo = w[i] & 0x55555555u, hi = (w[i] >> 1) & 0x55555555u;
            p11[i] = lo & hi;
            p10[i] = hi & ~lo;
            p00[i] = ~(lo | hi) & 0x55555555u;
         }
#pragma unroll
         for (int g = 0; g < FG; g++)
            if (f0 + g < nfolds) {
               const uint4 m = reinterpret_cast<const uint4 *>(masks + (size_t)(f0 + g) * pitch)[v];
               c[g][0] += __popc(p11[0] & m.x) + __popc(p11[1] & m.y) + __popc(p11[2] & m.z) + __popc(p11[3] & m.w);
               c[g][1] += __popc(p10[0] & m.x) + __popc(p10[1] & m.y) + __popc(p10[2] & m.z) + __popc(p10[3] & m.w);
               c[g][2] += __popc(p00[0] & m.x) + __popc(p00[1] & m.y) + __popc(p00[2] & m.z) + __popc(p00[3] & m.w);
            }
      }
#pragma unroll
      for (int g = 0; g < FG; g++)
#pragma unroll
         for (int d = 0; d < 3; d++) {
            uint32_t x = c[g][d];
            for (int off = 32; off > 0; off >>= 1) x += __shfl_down(x, off);
            if (lane == 0) red[wave][g * 3 + d] = x;
         }
      __syncthreads();
      if (threadIdx.x < FG * 3 && f0 + (int)threadIdx.x / 3 < nfolds)
         counts[((size_t)(f0 + threadIdx.x / 3) * P_g + snp) * 3 + threadIdx.x % 3] =
            red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
      __syncthreads();
   }
}

// mean / sd of the samples outside `fold` from the counts, by K1's formulas in K1's order (k_bed_stats; data.cpp:266-291)
__global__ __launch_bounds__(256) void k_fold_meansd(const uint32_t *__restrict__ counts, int nfolds, uint64_t P_g, int fold, int stand_method,
                                                     double *__restrict__ mean_out, double *__restrict__ sd_out)
{
   const uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x;
   if (j >= P_g) return;
   uint64_t n11 = 0, n10 = 0, n00 = 0;
   for (int f = 0; f < nfolds; f++)
      if (f != fold) {
         const uint32_t *p = counts + ((size_t)f * P_g + j) * 3;
         n11 += p[0];
         n10 += p[1];
         n00 += p[2];
      }
   const uint64_t ngood = n00 + n10 + n11;
   const double mean = (double)(2 * n00 + n10) / (double)ngood;
   const double pp = mean / 2.0;
   double sd;
   if (stand_method == 2)
      sd = sqrt(pp * (1 - pp));
   else
      sd = sqrt(2.0 * pp * (1 - pp));
   mean_out[j] = mean;
   sd_out[j] = sd;
}

// sum over the four waves of a 256-thread workgroup in a fixed order, the result in every thread
__device__ __forceinline__ double block_sum4(double v, double *red)
{
   for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
   if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
   __syncthreads();
   const double r = ((red[0] + red[1]) + red[2]) + red[3];
   __syncthreads();
   return r;
}

// util.cpp:24-110 (k_dense_standardise) with the statistics taken over the rows outside `fold` and applied to all N rows; one
// workgroup per phenotype; src / dst [k][N_pad]
__global__ __launch_bounds__(256) void k_cv_stand_y(const double *__restrict__ src, double *__restrict__ dst, uint64_t N_pad, uint64_t N,
                                                    const uint8_t *__restrict__ foldid, int fold, int method)
{
   const double *col = src + (uint64_t)blockIdx.x * N_pad;
   double *out = dst + (uint64_t)blockIdx.x * N_pad;
   __shared__ double red[4];
   double s1 = 0, s2 = 0, cnt = 0;
   for (uint64_t i = threadIdx.x; i < N; i += 256) {
      const double x = col[i];
      if (foldid[i] != fold && !isnan(x)) {
         const double xs = (method == 1) ? x - 1.0 : x;
         s1 += xs;
         s2 += xs * xs;
         cnt += 1.0;
      }
   }
   const double sum = block_sum4(s1, red), sum_sqr = block_sum4(s2, red), nj = block_sum4(cnt, red);
   double mean = 0.0, sd = 1.0;
   if (method == 0 || method == 4)
      mean = sum / nj;
   else if (method == 1) {
      const double varj = (sum_sqr - (sum * sum) / nj) / (nj - 1.0);
      mean = (sum + nj) / nj;
      sd = sqrt(varj);
   } else {
      mean = sum / nj;
      const double r = mean / 2.0;
      sd = sqrt((method == 2 ? 1.0 : 2.0) * r * (1.0 - r));
   }
   for (uint64_t i = threadIdx.x; i < N; i += 256) {
      const double x = col[i];
      double y;
      if (method == 0)
         y = isnan(x) ? mean : x;
      else if (method == 4)
         y = isnan(x) ? 0.0 : x - mean;
      else
         y = isnan(x) ? 0.0 : (sd > 1e-9 ? (x - mean) / sd : mean);
      out[i] = y;
   }
}

// K2's operand [N_pad][b] row-major: columns [c0, c0 + nc) of the standardised phenotypes * invdiv, the held-out and pad rows zero
__global__ void k_cv_operand(const double *__restrict__ Ys, uint64_t N_pad, uint64_t N, int c0, int nc, int b, double invdiv,
                             const uint8_t *__restrict__ foldid, int fold, double *__restrict__ blk)
{
   const uint64_t total = N_pad * b;
   for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (uint64_t)gridDim.x * 256) {
      const uint64_t s = i / b;
      const int c = (int)(i % b);
      blk[i] = (s < N && c < nc && foldid[s] != fold) ? Ys[(uint64_t)(c0 + c) * N_pad + s] * invdiv : 0.0;
   }
}

// non-zeros of column blockIdx.x of U [ncols][P]
__global__ __launch_bounds__(256) void k_cv_count_nz(const double *__restrict__ U, uint64_t P, uint32_t *__restrict__ nz)
{
   const double *u = U + (uint64_t)blockIdx.x * P;
   __shared__ uint32_t red[4];
   uint32_t n = 0;
   for (uint64_t i = threadIdx.x; i < P; i += 256) n += u[i] != 0;
   for (int off = 32; off > 0; off >>= 1) n += __shfl_down(n, off);
   if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = n;
   __syncthreads();
   if (threadIdx.x == 0) nz[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}

// the held-out rows of a K3 result block [N_pad][b] -> columns [col0, col0 + nc) of xpred (column-major, leading dimension N); NaN
// where the column's model did not converge (scca.R:503-509)
__global__ void k_cv_gather_x(const double *__restrict__ blk, int b, int nc, uint64_t N, const uint8_t *__restrict__ foldid, int fold,
                              const int *__restrict__ conv, int ndim, int col0, double *__restrict__ xpred)
{
   const uint64_t total = N * nc;
   for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (uint64_t)gridDim.x * 256) {
      const uint64_t s = i / nc;
      const int c = (int)(i % nc);
      if (foldid[s] != fold) continue;
      xpred[(uint64_t)(col0 + c) * N + s] = conv[(col0 + c) / ndim] ? blk[s * b + c] : __builtin_nan("");
   }
}

// ypred[s][col] = sum_c Ys[c][s] V[col][c] for the held-out rows s, in the order of c
__global__ void k_cv_ypred(const double *__restrict__ Ys, uint64_t N_pad, uint64_t N, int k, const double *__restrict__ V, int kp, int ncols,
                           const uint8_t *__restrict__ foldid, int fold, const int *__restrict__ conv, int ndim, double *__restrict__ ypred)
{
   const uint64_t total = N * ncols;
   for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (uint64_t)gridDim.x * 256) {
      const uint64_t col = i / N, s = i % N;
      if (foldid[s] != fold) continue;
      double a = 0;
      const double *v = V + col * kp;
      for (int c = 0; c < k; c++) a += Ys[(uint64_t)c * N_pad + s] * v[c];
      ypred[col * N + s] = conv[col / ndim] ? a : __builtin_nan("");
   }
}

// Pearson correlation of column blockIdx.x of xpred and ypred over all N rows: means first, then the centred sums.  NaN when a row
// is NaN (a model that did not converge) or a variance is zero (0 / 0).
__global__ __launch_bounds__(256) void k_cv_corr(const double *__restrict__ xpred, const double *__restrict__ ypred, uint64_t N,
                                                 double *__restrict__ corr)
{
   const double *x = xpred + (uint64_t)blockIdx.x * N, *y = ypred + (uint64_t)blockIdx.x * N;
   __shared__ double red[4];
   double sx = 0, sy = 0;
   for (uint64_t i = threadIdx.x; i < N; i += 256) {
      sx += x[i];
      sy += y[i];
   }
   const double mx = block_sum4(sx, red) / (double)N, my = block_sum4(sy, red) / (double)N;
   double sxx = 0, syy = 0, sxy = 0;
   for (uint64_t i = threadIdx.x; i < N; i += 256) {
      const double a = x[i] - mx, b = y[i] - my;
      sxx += a * a;
      syy += b * b;
      sxy += a * b;
   }
   sxx = block_sum4(sxx, red);
   syy = block_sum4(syy, red);
   sxy = block_sum4(sxy, red);
   if (threadIdx.x == 0) corr[blockIdx.x] = sxy / (sqrt(sxx) * sqrt(syy));
}

// block width of a K2 / K3 chunk of nc columns: 16, 32 or 64 (never 48: the exact-integer path has no gather kernels at that width and
// a context that meets it leaves its sparse / hybrid missing-call route for good)
int chunk_width(int nc) { return nc <= 16 ? 16 : nc <= 32 ? 32 : 64; }

unsigned grid_for(uint64_t total) { return (unsigned)std::min<uint64_t>(8192, std::max<uint64_t>(1, (total + 255) / 256)); }

// the context's standardisation while the folds swap it: saved before the first fold, put back on EVERY way out
struct StatsGuard {
   fpca_ctx *c;
   DevMem<double> own; // mean | sd | sumsq [P_pad each] | lut [4 P_pad]
   double trace_local;
   bool stats_done, missing_known;
   explicit StatsGuard(fpca_ctx *ctx)
      : c(ctx), own(7 * ctx->P_pad, "fpca_scca_cv", "the copy of the context's mean / sd"), trace_local(ctx->trace_local), stats_done(ctx->stats_done),
        missing_known(ctx->missing_known)
   {
      const size_t n = c->P_pad;
      double *save = own.p;
      const hipError_t e[4] = {hipMemcpyAsync(save, c->d_mean, n * sizeof(double), hipMemcpyDeviceToDevice, c->stream),
                               hipMemcpyAsync(save + n, c->d_sd, n * sizeof(double), hipMemcpyDeviceToDevice, c->stream),
                               hipMemcpyAsync(save + 2 * n, c->d_sumsq, n * sizeof(double), hipMemcpyDeviceToDevice, c->stream),
                               hipMemcpyAsync(save + 3 * n, c->d_lut, 4 * n * sizeof(double), hipMemcpyDeviceToDevice, c->stream)};
      for (hipError_t x : e)
         if (x != hipSuccess) throw Error(FPCA_EHIP, std::string("saving the context's mean / sd failed: ") + hipGetErrorString(x));
   }
   ~StatsGuard() // synchronise, copy back, synchronise; `own` is freed after this body
   {
      const size_t n = c->P_pad;
      const double *save = own.p;
      (void)hipStreamSynchronize(c->stream);
      (void)hipMemcpyAsync(c->d_mean, save, n * sizeof(double), hipMemcpyDeviceToDevice, c->stream);
      (void)hipMemcpyAsync(c->d_sd, save + n, n * sizeof(double), hipMemcpyDeviceToDevice, c->stream);
      (void)hipMemcpyAsync(c->d_sumsq, save + 2 * n, n * sizeof(double), hipMemcpyDeviceToDevice, c->stream);
      (void)hipMemcpyAsync(c->d_lut, save + 3 * n, 4 * n * sizeof(double), hipMemcpyDeviceToDevice, c->stream);
      (void)hipStreamSynchronize(c->stream);
      c->i8_scales_done = false;
      c->trace_local = trace_local;
      c->stats_done = stats_done;
      c->missing_known = missing_known;
   }
};

// fold ids -> the per-fold masks of k_fold_counts (host), and the fold sizes
void build_masks(const uint8_t *fold, uint64_t N, int nfolds, size_t pitch, std::vector<uint8_t> &masks, std::vector<uint64_t> &fsize)
{
   masks.assign((size_t)nfolds * pitch, 0);
   fsize.assign(nfolds, 0);
   for (uint64_t i = 0; i < N; i++) {
      masks[(size_t)fold[i] * pitch + i / 4] |= (uint8_t)(1u << (2 * (i % 4)));
      fsize[fold[i]]++;
   }
}

void check_folds(const fpca_ctx *c, const uint8_t *fold, int nfolds, const char *fn)
{
   if (c->dense)
      throw Error(FPCA_EINVAL, std::string(fn) + ": this context holds a dense matrix, of which only the standardised copy is kept; fold-wise "
                                                 "re-standardisation needs the packed genotypes (fpca_create, fpca_create_from_bed, synthetic)");
   if (nfolds < 2 || nfolds > 64) throw Error(FPCA_EINVAL, std::string(fn) + ": nfolds must be between 2 and 64, it is " + std::to_string(nfolds));
   for (uint64_t i = 0; i < c->N; i++)
      if (fold[i] >= nfolds)
         throw Error(FPCA_EINVAL, std::string(fn) + ": sample " + std::to_string(i) + " has fold id " + std::to_string((int)fold[i]) +
                                     ", the ids must be 0 .. nfolds - 1 = " + std::to_string(nfolds - 1));
}

void launch_fold_counts(fpca_ctx *c, const uint8_t *d_masks, int nfolds, uint32_t *d_counts, hipStream_t s)
{
   if (!c->P_g) return;
   hipLaunchKernelGGL(k_fold_counts, dim3((unsigned)c->P_g), dim3(256), 0, s, c->d_packed, c->pitch, d_masks, nfolds, c->P_g, d_counts);
   HIP_CHECK(hipGetLastError());
}

void launch_fold_meansd(fpca_ctx *c, const uint32_t *d_counts, int nfolds, int fold, double *d_mean, double *d_sd, hipStream_t s)
{
   if (!c->P_g) return;
   hipLaunchKernelGGL(k_fold_meansd, dim3((unsigned)((c->P_g + 255) / 256)), dim3(256), 0, s, d_counts, nfolds, c->P_g, fold, c->stand, d_mean, d_sd);
   HIP_CHECK(hipGetLastError());
}

struct CvArgs {
   const double *Y;
   int64_t ldy;
   int k;
   const uint8_t *fold;
   int nfolds;
   const double *l1;
   int n1;
   const double *l2;
   int n2;
   int ndim, stand_y, divisor, maxiter;
   double tol;
   const double *V0;
   int64_t ldv0, v0_stride;
   double warm;
   int opt_dim;
   double *corr, *nzero_x, *nzero_y;
   int *converged, *iters, *warm_iters;
   double *best_l1, *best_l2, *best_corr, *xpred, *ypred;
};

void scca_cv(fpca_ctx *c, const CvArgs &a)
{
   static const char *FN = "fpca_scca_cv";
   const uint64_t N = c->N, P = c->P_g;
   const int k = a.k, kp = pad16(k), ndim = a.ndim, nfolds = a.nfolds, ncell = a.n1 * a.n2, ncols = ncell * ndim;
   HIP_CHECK(hipSetDevice(c->device));
   hipStream_t s = c->stream;
   HIP_CHECK(hipStreamSynchronize(s));
   const bool timing = std::getenv("FPCA_TIMING") != nullptr;
   double t_ph[6] = {0, 0, 0, 0, 0, 0}; // fold counts, per-fold setup, K2, fits, K3 + gather, correlation
   long total_iters = 0;
   auto tl = std::chrono::steady_clock::now();
   auto lap = [&](int ph) {
      if (!timing) return;
      HIP_CHECK(hipStreamSynchronize(s));
      const auto now = std::chrono::steady_clock::now();
      if (ph >= 0) t_ph[ph] += std::chrono::duration<double>(now - tl).count();
      tl = now;
   };

   std::vector<uint8_t> masks;
   std::vector<uint64_t> fsize;
   build_masks(a.fold, N, nfolds, c->pitch, masks, fsize);
   uint64_t min_train = N;
   for (int f = 0; f < nfolds; f++) min_train = std::min(min_train, N - fsize[f]);
   if (min_train < 2) throw Error(FPCA_EINVAL, std::string(FN) + ": a fold leaves fewer than two samples to train on");
   const uint64_t maxdim = std::min<uint64_t>(std::min<uint64_t>(min_train, P), (uint64_t)k);
   if ((uint64_t)ndim > maxdim)
      throw Error(FPCA_EINVAL, std::string(FN) + ": You asked for " + std::to_string(ndim) + " dimensions, but only " + std::to_string(maxdim) +
                                  " allowed (the smallest training set has " + std::to_string(min_train) + " samples)");

   scca_free(c); // (C of an earlier fpca_scca_prepare would only take the room of this call's)
   ensure_stats(c);
   ensure_io(c);
   c->ensure(c->d_T, c->T_cap, (size_t)c->P_pad * MAX_BLOCKVEC);

   fpca_scca_state st;
   st.k = k;
   st.kp = kp;
   // (the state owns both, scca.hpp)
   st.d_C = static_cast<double *>(dev_alloc(std::max<size_t>((size_t)P * kp * sizeof(double), 8), FN,
                                            ("the " + std::to_string(P) + " x " + std::to_string(k) + " cross-product matrix").c_str()));
   st.d_flags = static_cast<int *>(dev_alloc(16, FN, "the iteration flags"));
   // (a buffer of no element is 8 bytes: every kernel is handed a pointer)
   DevMem<uint8_t> d_masks(masks.size(), FN, "the fold masks", 8), d_fold(N, FN, "the fold ids", 8);
   DevMem<uint32_t> d_counts((size_t)nfolds * P * 3, FN, "the per-fold genotype counts", 8);
   DevMem<double> d_Yraw((size_t)k * c->N_pad, FN, "the phenotypes", 8), d_Ys((size_t)k * c->N_pad, FN, "the standardised phenotypes", 8);
   DevMem<double> d_Uall((size_t)ncols * P, FN, "the workspace for a fold's U", 8), d_Vall((size_t)ncols * kp, FN, "the workspace for a fold's V", 8);
   DevMem<int> d_conv((size_t)ncell, FN, "the convergence flags", 8);
   DevMem<uint32_t> d_nz((size_t)ncols, FN, "the non-zero counts", 8);
   DevMem<double> d_xpred((size_t)ncols * N, FN, "xpred, the held-out projections of the genotypes", 8);
   DevMem<double> d_ypred((size_t)ncols * N, FN, "ypred, the held-out projections of the phenotypes", 8);
   DevMem<double> d_corr((size_t)ncols, FN, "the correlations", 8);

   HIP_CHECK(hipMemcpyAsync(d_masks.p, masks.data(), masks.size(), hipMemcpyHostToDevice, s));
   HIP_CHECK(hipMemcpyAsync(d_fold.p, a.fold, N, hipMemcpyHostToDevice, s));
   HIP_CHECK(hipMemcpy2DAsync(d_Yraw.p, c->N_pad * sizeof(double), a.Y, (size_t)a.ldy * sizeof(double), N * sizeof(double), k, hipMemcpyHostToDevice, s));
   HIP_CHECK(hipMemsetAsync(d_xpred.p, 0, (size_t)ncols * N * sizeof(double), s)); // scca.R:447-448
   HIP_CHECK(hipMemsetAsync(d_ypred.p, 0, (size_t)ncols * N * sizeof(double), s));
   HIP_CHECK(hipStreamSynchronize(s));
   lap(-1);
   launch_fold_counts(c, d_masks.p, nfolds, d_counts.p, s);
   lap(0);

   StatsGuard guard(c);
   std::vector<int> conv((size_t)nfolds * ncell, 0), iters((size_t)nfolds * ncell * ndim, 0), witers((size_t)nfolds * ndim, 0), fconv(ncell);
   std::vector<double> nzx((size_t)ncols, 0.0), nzy((size_t)ncols, 0.0), Vw((size_t)k * ndim), hV((size_t)ncols * kp);
   std::vector<uint32_t> hnz(ncols);
   for (int f = 0; f < nfolds; f++) {
      // the training standardisation of the genotypes, installed as fpca_set_meansd installs one
      launch_fold_meansd(c, d_counts.p, nfolds, f, c->d_mean, c->d_sd, s);
      kern::lut_from_meansd(c->d_mean, c->d_sd, P, c->d_lut, s);
      c->i8_scales_done = false;
      // ... and of the phenotypes
      hipLaunchKernelGGL(k_cv_stand_y, dim3((unsigned)k), dim3(256), 0, s, d_Yraw.p, d_Ys.p, c->N_pad, N, d_fold.p, f, a.stand_y);
      HIP_CHECK(hipGetLastError());
      st.invdiv = a.divisor == FPCA_DIVISOR_N1 ? 1.0 / std::sqrt((double)(N - fsize[f]) - 1.0) : 1.0;
      lap(1);
      // C_f = invdiv^2 X[T]' Y[T]: the chunked K2 pass of fpca_scca_prepare on an operand whose held-out rows are zero
      for (int c0 = 0; c0 < k; c0 += MAX_BLOCKVEC) {
         const int nc = std::min(MAX_BLOCKVEC, k - c0), bw = chunk_width(nc);
         hipLaunchKernelGGL(k_cv_operand, dim3(grid_for(c->N_pad * bw)), dim3(256), 0, s, d_Ys.p, c->N_pad, N, c0, nc, bw, st.invdiv, d_fold.p, f, c->d_io_a);
         HIP_CHECK(hipGetLastError());
         xt_dev(c, c->d_io_a, bw, s);
         scca_store_c(c->d_T, P, bw, nc, st.invdiv, st.d_C, kp, c0, s);
      }
      lap(2);
      // the warm start (scca.R:474-481), then the grid from its V
      const double *V0f = a.V0 + (size_t)f * a.v0_stride;
      const double *Vs = V0f;
      int64_t ldvs = a.ldv0;
      SccaDevFit fit;
      if (a.warm >= 0) {
         scca_fit_dev(c, &st, a.warm, a.warm, ndim, a.maxiter, a.tol, V0f, a.ldv0, fit);
         HIP_CHECK(hipMemcpy2DAsync(Vw.data(), (size_t)k * sizeof(double), fit.dV, (size_t)kp * sizeof(double), (size_t)k * sizeof(double), ndim,
                                    hipMemcpyDeviceToHost, s));
         HIP_CHECK(hipStreamSynchronize(s));
         for (int q = 0; q < ndim; q++) {
            witers[(size_t)f * ndim + q] = fit.iters[q];
            total_iters += fit.iters[q];
         }
         Vs = Vw.data();
         ldvs = k;
      }
      for (int cell = 0; cell < ncell; cell++) {
         scca_fit_dev(c, &st, a.l1[cell / a.n2], a.l2[cell % a.n2], ndim, a.maxiter, a.tol, Vs, ldvs, fit);
         HIP_CHECK(hipMemcpyAsync(d_Uall.p + (size_t)cell * ndim * P, fit.dU, (size_t)ndim * P * sizeof(double), hipMemcpyDeviceToDevice, s));
         HIP_CHECK(hipMemcpyAsync(d_Vall.p + (size_t)cell * ndim * kp, fit.dV, (size_t)ndim * kp * sizeof(double), hipMemcpyDeviceToDevice, s));
         fconv[cell] = conv[(size_t)f * ncell + cell] = fit.converged;
         for (int q = 0; q < ndim; q++) {
            iters[((size_t)f * ncell + cell) * ndim + q] = fit.iters[q];
            total_iters += fit.iters[q];
         }
      }
      HIP_CHECK(hipMemcpyAsync(d_conv.p, fconv.data(), (size_t)ncell * sizeof(int), hipMemcpyHostToDevice, s));
      hipLaunchKernelGGL(k_cv_count_nz, dim3((unsigned)ncols), dim3(256), 0, s, d_Uall.p, P, d_nz.p);
      HIP_CHECK(hipGetLastError());
      HIP_CHECK(hipMemcpyAsync(hnz.data(), d_nz.p, (size_t)ncols * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
      HIP_CHECK(hipMemcpyAsync(hV.data(), d_Vall.p, (size_t)ncols * kp * sizeof(double), hipMemcpyDeviceToHost, s));
      HIP_CHECK(hipStreamSynchronize(s));
      for (int col = 0; col < ncols; col++) { // scca.R:516-523: the mean over the folds
         nzx[col] += (double)hnz[col];
         int nz = 0;
         for (int i = 0; i < k; i++) nz += hV[(size_t)col * kp + i] != 0;
         nzy[col] += (double)nz;
      }
      lap(3);
      // the held-out predictions (scca.R:504-505): K3 on every model's U, at most 64 columns a pass
      if (fsize[f]) {
         for (int c0 = 0; c0 < ncols; c0 += MAX_BLOCKVEC) {
            const int nc = std::min(MAX_BLOCKVEC, ncols - c0), bw = chunk_width(nc);
            kern::colmajor_to_t(d_Uall.p + (size_t)c0 * P, P, P, c->P_pad, bw, nc, c->d_T, s);
            x_dev(c, bw, c->d_io_b, s);
            hipLaunchKernelGGL(k_cv_gather_x, dim3(grid_for(N * nc)), dim3(256), 0, s, c->d_io_b, bw, nc, N, d_fold.p, f, d_conv.p, ndim, c0, d_xpred.p);
            HIP_CHECK(hipGetLastError());
         }
         hipLaunchKernelGGL(k_cv_ypred, dim3(grid_for(N * ncols)), dim3(256), 0, s, d_Ys.p, c->N_pad, N, k, d_Vall.p, kp, ncols, d_fold.p, f, d_conv.p, ndim, d_ypred.p);
         HIP_CHECK(hipGetLastError());
      }
      HIP_CHECK(hipStreamSynchronize(s)); // (fconv is reused by the next fold)
      lap(4);
   }
   hipLaunchKernelGGL(k_cv_corr, dim3((unsigned)ncols), dim3(256), 0, s, d_xpred.p, d_ypred.p, N, d_corr.p);
   HIP_CHECK(hipGetLastError());
   std::vector<double> hcorr(ncols);
   HIP_CHECK(hipMemcpyAsync(hcorr.data(), d_corr.p, (size_t)ncols * sizeof(double), hipMemcpyDeviceToHost, s));
   HIP_CHECK(hipStreamSynchronize(s));
   lap(5);

   // results: device columns are (cell, q) = cell * ndim + q; corr / nzero_* go out as [q][i][j]
   const double nan = std::numeric_limits<double>::quiet_NaN();
   for (int cell = 0; cell < ncell; cell++)
      for (int q = 0; q < ndim; q++) {
         const size_t o = (size_t)q * ncell + cell, col = (size_t)cell * ndim + q;
         if (a.corr) a.corr[o] = hcorr[col];
         if (a.nzero_x) a.nzero_x[o] = nzx[col] / nfolds;
         if (a.nzero_y) a.nzero_y[o] = nzy[col] / nfolds;
      }
   if (a.converged) std::copy(conv.begin(), conv.end(), a.converged);
   if (a.iters) std::copy(iters.begin(), iters.end(), a.iters);
   if (a.warm_iters) std::copy(witers.begin(), witers.end(), a.warm_iters);
   // scca.R:538-547: the largest finite correlation of dimension opt_dim; ties in which()'s order, lambda1's index fastest
   double best = nan, b1 = nan, b2 = nan;
   for (int j = 0; j < a.n2; j++)
      for (int i = 0; i < a.n1; i++) {
         const double r = hcorr[(size_t)(i * a.n2 + j) * ndim + (a.opt_dim - 1)];
         if (std::isfinite(r) && (std::isnan(best) || r > best)) {
            best = r;
            b1 = a.l1[i];
            b2 = a.l2[j];
         }
      }
   if (a.best_corr) *a.best_corr = best;
   if (a.best_l1) *a.best_l1 = b1;
   if (a.best_l2) *a.best_l2 = b2;
   if (a.xpred) HIP_CHECK(hipMemcpy(a.xpred, d_xpred.p, (size_t)ncols * N * sizeof(double), hipMemcpyDeviceToHost));
   if (a.ypred) HIP_CHECK(hipMemcpy(a.ypred, d_ypred.p, (size_t)ncols * N * sizeof(double), hipMemcpyDeviceToHost));
   if (timing)
      std::fprintf(stderr,
                   "[fpca] scca_cv: fold counts %.3f ms, per-fold setup %.3f ms, K2 %.3f ms, fits %.3f ms (%ld iterations), K3 + gather %.3f ms, "
                   "correlation %.3f ms\n",
                   t_ph[0] * 1e3, t_ph[1] * 1e3, t_ph[2] * 1e3, t_ph[3] * 1e3, total_iters, t_ph[4] * 1e3, t_ph[5] * 1e3);
}

} // namespace

extern "C" int fpca_scca_cv(fpca_ctx *ctx, const double *Y, int64_t ldy, int k, const uint8_t *fold, int nfolds, const double *lambda1, int n1,
                            const double *lambda2, int n2, int ndim, int stand_y, int divisor, int maxiter, double tol, const double *V0,
                            int64_t ldv0, int64_t v0_stride, double warm_lambda, int opt_dim, double *corr, double *nzero_x, double *nzero_y,
                            int *converged, int *iters, int *warm_iters, double *best_lambda1, double *best_lambda2, double *best_corr,
                            double *xpred, double *ypred)
{
   return guarded([&] {
      static const std::string FN = "fpca_scca_cv: ";
      if (!ctx) throw Error(FPCA_EINVAL, "bad argument to fpca_scca_cv (NULL context)");
      if (!Y || !fold || !lambda1 || !lambda2 || !V0) throw Error(FPCA_EINVAL, "bad argument to fpca_scca_cv (NULL pointer: Y, fold, lambda1, lambda2 and V0 are required)");
      scca_check_single(ctx, "fpca_scca_cv");
      check_folds(ctx, fold, nfolds, "fpca_scca_cv");
      if (k < 1) throw Error(FPCA_EINVAL, FN + "at least one phenotype is needed (k >= 1)");
      if (k > SCCA_MAX_K) throw Error(FPCA_EINVAL, FN + std::to_string(k) + " phenotypes; at most " + std::to_string(SCCA_MAX_K) + " are supported");
      if (ldy < (int64_t)ctx->N) throw Error(FPCA_EINVAL, FN + "ldy is smaller than the number of samples");
      if (stand_y < FPCA_STANDARDISE_NONE || stand_y > FPCA_STANDARDISE_CENTER)
         throw Error(FPCA_EINVAL, FN + "unknown phenotype standardisation " + std::to_string(stand_y));
      if (n1 < 1 || n2 < 1) throw Error(FPCA_EINVAL, FN + "at least one lambda1 and one lambda2 are needed");
      if ((int64_t)n1 * n2 > 4096) throw Error(FPCA_EINVAL, FN + "at most 4096 penalty pairs are supported");
      for (int i = 0; i < n1; i++)
         if (!(lambda1[i] >= 0) || !std::isfinite(lambda1[i])) throw Error(FPCA_EINVAL, FN + "lambda1 must be non-negative and finite");
      for (int i = 0; i < n2; i++)
         if (!(lambda2[i] >= 0) || !std::isfinite(lambda2[i])) throw Error(FPCA_EINVAL, FN + "lambda2 must be non-negative and finite");
      if (!std::isfinite(warm_lambda) && !(warm_lambda < 0)) throw Error(FPCA_EINVAL, FN + "the warm-start penalty must be finite (negative: no warm start)");
      if (ndim < 1) throw Error(FPCA_EINVAL, FN + "ndim can't be less than 1");
      if (opt_dim < 1 || opt_dim > ndim) throw Error(FPCA_EINVAL, FN + "opt_dim must be between 1 and ndim");
      if (!(tol > 0)) throw Error(FPCA_EINVAL, FN + "tol must be positive");
      if (maxiter < 1) throw Error(FPCA_EINVAL, FN + "maxiter must be at least 1");
      if (ldv0 < k) throw Error(FPCA_EINVAL, FN + "ldv0 is smaller than the number of phenotypes");
      if (v0_stride < ldv0 * (int64_t)ndim && v0_stride != 0)
         throw Error(FPCA_EINVAL, FN + "the fold stride of V0 is smaller than one k x ndim matrix (0: every fold starts from the same one)");
      for (int f = 0; f < nfolds; f++)
         for (int j = 0; j < ndim; j++)
            for (int i = 0; i < k; i++)
               if (!std::isfinite(V0[(size_t)f * v0_stride + (size_t)j * ldv0 + i])) throw Error(FPCA_EINVAL, FN + "V0 holds a value that is not finite");
      scca_cv(ctx, CvArgs{Y, ldy, k, fold, nfolds, lambda1, n1, lambda2, n2, ndim, stand_y, divisor, maxiter, tol, V0, ldv0, v0_stride, warm_lambda, opt_dim,
                          corr, nzero_x, nzero_y, converged, iters, warm_iters, best_lambda1, best_lambda2, best_corr, xpred, ypred});
   });
}

extern "C" int fpca_debug_fold_stats(fpca_ctx *ctx, const uint8_t *fold, int nfolds, uint32_t *counts, int which_fold, double *mean_sd)
{
   return guarded([&] {
      if (!ctx || !fold) throw Error(FPCA_EINVAL, "bad argument to fpca_debug_fold_stats (NULL pointer)");
      check_folds(ctx, fold, nfolds, "fpca_debug_fold_stats");
      if (mean_sd && (which_fold < 0 || which_fold >= nfolds)) throw Error(FPCA_EINVAL, "fpca_debug_fold_stats: which_fold must be 0 .. nfolds - 1");
      HIP_CHECK(hipSetDevice(ctx->device));
      hipStream_t s = ctx->stream;
      const uint64_t P = ctx->P_g;
      std::vector<uint8_t> masks;
      std::vector<uint64_t> fsize;
      build_masks(fold, ctx->N, nfolds, ctx->pitch, masks, fsize);
      static const char *FN = "fpca_debug_fold_stats";
      DevMem<uint8_t> d_masks(masks.size(), FN, "the fold masks", 8);
      DevMem<uint32_t> d_counts((size_t)nfolds * P * 3, FN, "the per-fold genotype counts", 8);
      DevMem<double> d_ms(2 * (size_t)P, FN, "mean / sd", 8);
      HIP_CHECK(hipMemcpyAsync(d_masks.p, masks.data(), masks.size(), hipMemcpyHostToDevice, s));
      launch_fold_counts(ctx, d_masks.p, nfolds, d_counts.p, s);
      if (counts && P) HIP_CHECK(hipMemcpyAsync(counts, d_counts.p, (size_t)nfolds * P * 3 * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
      if (mean_sd && P) {
         launch_fold_meansd(ctx, d_counts.p, nfolds, which_fold, d_ms.p, d_ms.p + P, s);
         HIP_CHECK(hipMemcpyAsync(mean_sd, d_ms.p, 2 * (size_t)P * sizeof(double), hipMemcpyDeviceToHost, s));
      }
      HIP_CHECK(hipStreamSynchronize(s));
   });
}
