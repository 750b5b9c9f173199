// ucca.hip -- per-SNP association with k phenotypes (RandomPCA::ucca, randompca.cpp:530-625 + wilks, :103-119; plink.multivariate):
// fpca_ucca and the two builds of its F tail on their own: fpca_debug_f_sf (host) and fpca_debug_f_sf_dev (device).
//
// The reference takes the SVD Y = U D V' of the standardised phenotypes and, SNP by SNP, r2_j = |sum (cov(x_j, Y) V sqrt(n-1) / d)^2|
// / var(x_j).  Since V D^-2 V' = (Y'Y)^-1 and 1'Y_c = 0 (Y_c = Y - 1 mean(Y)'), that is
//     r2_j = || W' x_j ||^2 / || x_j - mean(x_j) 1 ||^2,     W = Y_c R^-1,  Y = Q R (thin QR of the standardised, not re-centred, Y)
// -- for every --standy, "none" on uncentred phenotypes included (there it is the reference's formula, not lm's R^2).  So the whole
// scan is ONE product X_g' [W | 1]: the context's K2 pass (xt_dev: exact int8, fp64 or fp32, whatever the context runs), fed in
// chunks of at most 64 columns; the ones column gives sum_i x_ij from the same pass, and sum_i x_ij^2 is K1's (or the dense
// standardisation's) d_sumsq.  Two small kernels finish it on the device:
//   k_ucca_accum   after each chunk: num_j += sum_m T_jm^2 over the chunk's W columns (T where K2 left it, [P_pad][b] row-major)
//   k_ucca_finish  den_j = sumsq_j - (sum x_j)^2 / N, r2, then R, Fstat, P (f_tail.hpp) -> P_g x 3 column-major
// Only those 24 bytes per SNP cross PCIe.  Edge rules: den_j = 0 (monomorphic / all-missing SNP) -> NaN, NaN, NaN; r2 >= 1 after
// rounding -> R = 1, Fstat = +inf, P = 0.  The host part is the phenotype side: upload, kern::dense_standardise (the one
// restatement of util.cpp:24-110 in the tree), download, Householder QR in fp64 (Y'Y is never formed), W = Y_c R^-1.
#include <algorithm>
#include <cmath>
#include <memory>

#include "ctx.hpp"
#include "f_tail.hpp"
#include "../../include/fpca_debug.h"

using namespace fpca;

namespace {

// den_j at or below this fraction of sum x_j^2 is rounding noise of a constant column (a dense column with sd <= 1e-9 keeps its
// mean): the SNP has no variance
constexpr double DEN_TOL = 16 * 2.220446049250313e-16;

// 16 lanes per SNP row, 16 rows per workgroup: a row group reads 128 contiguous bytes of T per step
__global__ __launch_bounds__(256) void k_ucca_accum(const double *__restrict__ T, uint64_t P_g, int b, int ncw, int ones_col,
                                                   double *__restrict__ num, double *__restrict__ sumx, int first)
{
   const uint64_t j = (uint64_t)blockIdx.x * 16 + (threadIdx.x >> 4);
   const int l = threadIdx.x & 15;
   if (j >= P_g) return; // (whole 16-lane groups leave together: the shuffles below stay within one group)
   const double *row = T + j * (uint64_t)b;
   double s = 0;
   for (int c = l; c < b; c += 16) {
      const double t = row[c];
      if (c < ncw) s += t * t;
      if (c == ones_col) sumx[j] = t;
   }
   for (int off = 8; off > 0; off >>= 1) s += __shfl_xor(s, off, 16);
   if (l == 0) num[j] = first ? s : num[j] + s;
}

__global__ __launch_bounds__(64) void k_ucca_finish(const double *__restrict__ num, const double *__restrict__ sumx,
                                                    const double *__restrict__ sumsq, uint64_t P_g, uint64_t N, int k,
                                                    double *__restrict__ res)
{
   const uint64_t j = (uint64_t)blockIdx.x * 64 + threadIdx.x;
   if (j >= P_g) return;
   const double ss = sumsq[j], sx = sumx[j];
   const double den = ss - sx * sx / (double)N;
   double R, F, P;
   if (!(den > DEN_TOL * ss)) {
      R = F = P = NAN;
   } else {
      const double r2 = num[j] / den;
      ftail::f_sf(r2, N, k, &F, &P);
      R = r2 >= 1.0 ? 1.0 : sqrt(r2);
   }
   res[j] = R;
   res[P_g + j] = F;
   res[2 * P_g + j] = P;
}

// fpca_debug_f_sf_dev: the device build of the F tail alone, one lane per r2, called as k_ucca_finish calls it
__global__ __launch_bounds__(256) void k_f_sf(const double *__restrict__ r2, uint64_t count, uint64_t n, int k, double *__restrict__ F,
                                              double *__restrict__ P)
{
   const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
   if (i >= count) return;
   double f, p;
   ftail::f_sf(r2[i], n, k, &f, &p);
   F[i] = f;
   P[i] = p;
}

// Householder QR of the N x k column-major A (overwritten): the diagonal and upper triangle of R, k x k column-major
void householder_r(double *A, uint64_t N, int k, std::vector<double> &R)
{
   R.assign((size_t)k * k, 0.0);
   for (int j = 0; j < k; j++) {
      double *v = A + (size_t)j * N + j;
      const uint64_t m = N - j;
      double nrm2 = 0;
      for (uint64_t i = 0; i < m; i++) nrm2 += v[i] * v[i];
      const double nrm = std::sqrt(nrm2);
      const double alpha = v[0] > 0 ? -nrm : nrm;
      R[(size_t)j * k + j] = alpha;
      if (nrm == 0) continue; // (a zero column: rank deficient, refused by the caller)
      const double v0 = v[0] - alpha, vn2 = nrm2 - v[0] * v[0] + v0 * v0;
      v[0] = v0;
      for (int c = j + 1; c < k; c++) {
         double *a = A + (size_t)c * N + j;
         double s = 0;
         for (uint64_t i = 0; i < m; i++) s += v[i] * a[i];
         const double f = 2.0 * s / vn2;
         for (uint64_t i = 0; i < m; i++) a[i] -= f * v[i];
         R[(size_t)c * k + j] = a[0];
      }
   }
}

} // namespace

namespace fpca {

void ucca(fpca_ctx *c, const double *Y, int64_t ldy, int k, int stand_y, double *res, int64_t ldres)
{
   const uint64_t N = c->N, P = c->P_g;
   HIP_CHECK(hipSetDevice(c->device));
   ensure_stats(c);
   if (!c->dense && !c->missing_known)
      throw Error(FPCA_EINVAL, "fpca_ucca needs the context's own SNP statistics (mean/sd were preloaded with fpca_set_meansd)");
   hipStream_t s = c->stream;

   // 1. phenotypes: upload as rows of a [k][N_pad] image, standardise there (util.cpp:24-110), download the standardised N x k
   std::vector<double> Ys((size_t)N * k);
   {
      DevMem<double> dY((size_t)k * c->N_pad, "fpca_ucca", "the phenotypes"), dstat(3 * (size_t)k, "fpca_ucca", "the phenotype statistics");
      HIP_CHECK(hipMemcpy2DAsync(dY.p, c->N_pad * sizeof(double), Y, (size_t)ldy * sizeof(double), N * sizeof(double), k, hipMemcpyHostToDevice, s));
      kern::dense_standardise(dY.p, c->N_pad, N, k, stand_y, dstat.p, dstat.p + k, dstat.p + 2 * k, s);
      HIP_CHECK(hipMemcpy2DAsync(Ys.data(), N * sizeof(double), dY.p, c->N_pad * sizeof(double), N * sizeof(double), k, hipMemcpyDeviceToHost, s));
      HIP_CHECK(hipStreamSynchronize(s));
   }
   // column means of the standardised Y (blocked sums)
   std::vector<double> ybar(k);
   for (int j = 0; j < k; j++) ybar[j] = blocked_sum(Ys.data() + (size_t)j * N, N) / (double)N;

   // 2. R of the thin QR of Y (on a copy: Ys is needed again for Y_c)
   std::vector<double> R;
   {
      std::vector<double> A(Ys);
      householder_r(A.data(), N, k, R);
   }
   double rmax = 0;
   for (int j = 0; j < k; j++) rmax = std::max(rmax, std::fabs(R[(size_t)j * k + j]));
   for (int j = 0; j < k; j++)
      if (!(std::fabs(R[(size_t)j * k + j]) > 1e-12 * rmax))
         throw Error(FPCA_EINVAL, "the standardised phenotype matrix is rank deficient (column " + std::to_string(j + 1) +
                                      " is a linear combination of the others, or constant)");

   // 3. B = [W | 1], W = Y_c R^-1 column by column: W_j = (Y_c,j - sum_{i<j} R_ij W_i) / R_jj
   const int ncol = k + 1;
   std::vector<double> B((size_t)N * ncol);
   for (int j = 0; j < k; j++) {
      double *w = B.data() + (size_t)j * N;
      const double *y = Ys.data() + (size_t)j * N;
      for (uint64_t i = 0; i < N; i++) w[i] = y[i] - ybar[j];
      for (int q = 0; q < j; q++) {
         const double r = R[(size_t)j * k + q];
         const double *wq = B.data() + (size_t)q * N;
         for (uint64_t i = 0; i < N; i++) w[i] -= r * wq[i];
      }
      const double inv = 1.0 / R[(size_t)j * k + j];
      for (uint64_t i = 0; i < N; i++) w[i] *= inv;
   }
   std::fill(B.begin() + (size_t)k * N, B.end(), 1.0);

   // 4. the chunked K2 pass X_g' B, the numerator accumulated after each chunk, then the statistics
   ensure_io(c);
   DevMem<double> dnum(c->P_pad, "fpca_ucca", "the numerators"), dsumx(c->P_pad, "fpca_ucca", "the column sums"), dres(3 * P, "fpca_ucca", "the statistics");
   for (int c0 = 0; c0 < ncol; c0 += MAX_BLOCKVEC) {
      const int nc = std::min(MAX_BLOCKVEC, ncol - c0), bw = pad16(nc);
      const int ncw = std::max(0, std::min(k, c0 + nc) - c0), ones_col = (k < c0 + nc) ? k - c0 : -1;
      c->ensure(c->d_stage, c->stage_cap, (size_t)std::max(N, P) * nc);
      HIP_CHECK(hipMemcpy2DAsync(c->d_stage, N * sizeof(double), B.data() + (size_t)c0 * N, N * sizeof(double), N * sizeof(double), nc,
                                 hipMemcpyHostToDevice, s));
      kern::colmajor_to_block(c->d_stage, N, N, c->N_pad, bw, nc, c->d_io_a, s);
      xt_dev(c, c->d_io_a, bw, s);
      if (P) {
         hipLaunchKernelGGL(k_ucca_accum, dim3((unsigned)((P + 15) / 16)), dim3(256), 0, s, c->d_T, P, bw, ncw, ones_col, dnum.p, dsumx.p,
                            c0 == 0 ? 1 : 0);
         HIP_CHECK(hipGetLastError());
      }
   }
   if (P) {
      hipLaunchKernelGGL(k_ucca_finish, dim3((unsigned)((P + 63) / 64)), dim3(64), 0, s, dnum.p, dsumx.p, c->d_sumsq, P, N, k, dres.p);
      HIP_CHECK(hipGetLastError());
      HIP_CHECK(hipMemcpy2DAsync(res, (size_t)ldres * sizeof(double), dres.p, P * sizeof(double), P * sizeof(double), 3, hipMemcpyDeviceToHost, s));
   }
   HIP_CHECK(hipStreamSynchronize(s));
}

} // namespace fpca

extern "C" int fpca_ucca(fpca_ctx *ctx, const double *Y, int64_t ldy, int k, int stand_y, double *res, int64_t ldres)
{
   return guarded([&] {
      if (!ctx || !Y || !res) throw Error(FPCA_EINVAL, "bad argument to fpca_ucca (NULL pointer)");
      refuse_masked(ctx, "fpca_ucca");
      if (k < 1) throw Error(FPCA_EINVAL, "fpca_ucca needs at least one phenotype (k >= 1)");
      if ((uint64_t)k + 2 > ctx->N)
         throw Error(FPCA_EINVAL, "fpca_ucca: " + std::to_string(k) + " phenotypes need at least " + std::to_string((uint64_t)k + 2) +
                                      " samples (n - k - 1 >= 1), the context has " + std::to_string(ctx->N));
      if (ldy < (int64_t)ctx->N) throw Error(FPCA_EINVAL, "fpca_ucca: ldy is smaller than the number of samples");
      if (ldres < (int64_t)ctx->P_g) throw Error(FPCA_EINVAL, "fpca_ucca: ldres is smaller than the number of SNPs of the context");
      if (stand_y < FPCA_STANDARDISE_NONE || stand_y > FPCA_STANDARDISE_CENTER)
         throw Error(FPCA_EINVAL, "fpca_ucca: unknown phenotype standardisation " + std::to_string(stand_y));
      ucca(ctx, Y, ldy, k, stand_y, res, ldres);
   });
}

extern "C" int fpca_debug_f_sf(double r2, uint64_t n, int k, double *F, double *P)
{
   return guarded([&] {
      if (!F || !P || k < 1 || (uint64_t)k + 2 > n) throw Error(FPCA_EINVAL, "bad argument to fpca_debug_f_sf (needs k >= 1, n >= k + 2)");
      ftail::f_sf(r2, n, k, F, P);
   });
}

extern "C" int fpca_debug_f_sf_dev(const double *r2, uint64_t count, uint64_t n, int k, double *F, double *P)
{
   return guarded([&] {
      if (!F || !P || k < 1 || (uint64_t)k + 2 > n) throw Error(FPCA_EINVAL, "bad argument to fpca_debug_f_sf_dev (needs k >= 1, n >= k + 2)");
      if (!count) return;
      if (!r2) throw Error(FPCA_EINVAL, "bad argument to fpca_debug_f_sf_dev (NULL pointer)");
      if (count > (uint64_t)1 << 31) throw Error(FPCA_EINVAL, "fpca_debug_f_sf_dev: more than 2^31 values");
      DevMem<double> buf(3 * (size_t)count, "fpca_debug_f_sf_dev", "the values and their statistics");
      double *dr2 = buf.p, *dF = dr2 + count, *dP = dF + count;
      HIP_CHECK(hipMemcpy(dr2, r2, count * sizeof(double), hipMemcpyHostToDevice));
      hipLaunchKernelGGL(k_f_sf, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, nullptr, dr2, count, n, k, dF, dP);
      HIP_CHECK(hipGetLastError());
      HIP_CHECK(hipMemcpy(F, dF, count * sizeof(double), hipMemcpyDeviceToHost)); // (the null stream: after the kernel)
      HIP_CHECK(hipMemcpy(P, dP, count * sizeof(double), hipMemcpyDeviceToHost));
   });
}
