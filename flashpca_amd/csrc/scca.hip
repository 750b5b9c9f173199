// scca.hip -- sparse canonical correlation analysis of the genotypes with k phenotypes (RandomPCA::scca(Data&, ...),
// randompca.cpp:387-528; norm_thresh / soft_thresh, :225-245; the R function scca()): fpca_scca_prepare and fpca_scca_fit.
//
// The reference's loop is, per canonical dimension j and per iteration,
//     u <- invdiv X'(Yh v_j)   Gram-Schmidt against U[:, <j]   u <- norm_thresh(u, lambda1)
//     v <- invdiv Yh'(X u)     Gram-Schmidt against V[:, <j]   v <- norm_thresh(v, lambda2)
// with Yh = standardised Y * invdiv: two passes over the .bed per iteration.  X and Yh never change, so with
//     C = invdiv X' Yh        (P x k, fp64, resident in HBM)
// the two products are C v and C'u and d_j = u'C v.  fpca_scca_prepare forms C with ONE chunked K2 pass (xt_dev, as fpca_ucca drives it);
// fpca_scca_fit iterates on C alone and ends with ONE K3 pass, Px = invdiv X U.  One iteration is five plain launches (four in
// dimension 0) on the context's stream:
//   k_scca_cv      t = C v, 16 lanes per row of C; per workgroup the partial sums of ||t||^2 and of t.U_q, q < j
//   k_scca_gs      (j > 0) c_q from the dots and the fixed Gram matrix G of U[:, <j] by the triangular recurrence, t -= sum c_q U_q,
//                  partial sums of the new ||t||^2
//   k_scca_thresh  t <- soft_thresh(t / ||t||, lambda1), partial sums of its squared norm
//   k_scca_update  u = t / ||t||, max |u - u_old|, max |u|, U[:, j] = u; partial sums of C'u over the rows with u != 0
//   k_scca_v       one workgroup, everything of length k: w = C'u, Gram-Schmidt on v, norm_thresh, max |v - v_old|, d = w.v, the
//                  convergence decision, the iteration counter
// A sum over workgroups is finished by every workgroup of the NEXT launch, which adds the partials in a fixed order: the kernel
// boundary is the only synchronisation between workgroups, nothing spins, and a fit is reproducible bit for bit.  u, v, the flags
// and the counter live in device memory; once k_scca_v has set `done` every later launch returns at once, so the host enqueues
// iterations in batches and reads the two words between batches -- results are those of stopping on the exact iteration.
// C is [P][k_pad] row-major (k_pad = k rounded up to 16, the pad columns zero): C v reads 128 contiguous bytes per 16-lane
// group and step, C'u is a column sum over the same rows.  Everything is fp64.
#include <algorithm>
#include <cmath>
#include <memory>

#include "ctx.hpp"
#include "scca.hpp"

using namespace fpca;

namespace {

constexpr int RB = 256;    // rows of C per workgroup (16 passes of 16 rows, 16 lanes per row)
constexpr int BATCH = 16;  // iterations enqueued between two looks at the flags
constexpr int DONE_CONVERGED = 1, DONE_U_ZERO = 2, DONE_V_ZERO = 3;

// sums / maxima over the NW waves of a workgroup in a fixed order, the result in every thread (red: NW doubles of LDS)
template <int NW> __device__ __forceinline__ double block_sum(double v, double *red)
{
   for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
   if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
   __syncthreads();
   double r = 0;
#pragma unroll
   for (int w = 0; w < NW; w++) r += red[w];
   __syncthreads();
   return r;
}

template <int NW> __device__ __forceinline__ double block_max(double v, double *red)
{
   for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off, 64));
   if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
   __syncthreads();
   double r = red[0];
#pragma unroll
   for (int w = 1; w < NW; w++) r = fmax(r, red[w]);
   __syncthreads();
   return r;
}

// sum of part[i * stride], i < n, finished by the whole workgroup
template <int NW> __device__ __forceinline__ double sum_partials(const double *part, int n, int stride, double *red)
{
   double s = 0;
   for (int i = threadIdx.x; i < n; i += 64 * NW) s += part[(size_t)i * stride];
   return block_sum<NW>(s, red);
}

// T (where K2 left a chunk, [P_pad][b] row-major) -> columns [c0, min(c0 + b, kp)) of C, scaled; columns >= nc of the chunk are C's zero pad
__global__ __launch_bounds__(256) void k_scca_store_c(const double *__restrict__ T, uint64_t P_g, int b, int nc, double scale,
                                                      double *__restrict__ Cm, int kp, int c0)
{
   const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
   if (i >= P_g * (uint64_t)b) return;
   const uint64_t j = i / b;
   const int c = (int)(i % b);
   if (c0 + c >= kp) return; // (a chunk wider than C's own pad: fpca_scca_cv never passes 48 columns to K2)
   Cm[j * kp + c0 + c] = c < nc ? scale * T[i] : 0.0;
}

// t = C v; part[blk][0] = sum t^2, part[blk][1 + q] = sum t U_q (q < j) over the workgroup's rows
__global__ __launch_bounds__(256) void k_scca_cv(const double *__restrict__ Cm, uint64_t P, int kp, const double *v, const double *U, int j,
                                                 double *t, double *part, int pstride, const int *flags)
{
   __shared__ double tl[RB];
   __shared__ double red[4];
   if (flags[0]) return;
   const uint64_t row0 = (uint64_t)blockIdx.x * RB;
   const int g = threadIdx.x >> 4, l = threadIdx.x & 15;
   for (int pass = 0; pass < RB / 16; pass++) {
      const uint64_t r = row0 + pass * 16 + g;
      double s = 0;
      if (r < P) {
         const double *row = Cm + r * kp;
         for (int c = l; c < kp; c += 16) s += row[c] * v[c];
      }
      for (int off = 8; off > 0; off >>= 1) s += __shfl_xor(s, off, 16);
      if (l == 0) tl[pass * 16 + g] = s;
   }
   __syncthreads();
   const uint64_t r = row0 + threadIdx.x;
   const bool in = r < P;
   const double ti = in ? tl[threadIdx.x] : 0.0;
   if (in) t[r] = ti;
   double *out = part + (size_t)blockIdx.x * pstride;
   const double ss = block_sum<4>(ti * ti, red);
   if (threadIdx.x == 0) out[0] = ss;
   for (int q = 0; q < j; q++) {
      const double a = block_sum<4>(in ? ti * U[(size_t)q * P + r] : 0.0, red);
      if (threadIdx.x == 0) out[1 + q] = a;
   }
}

// the reference's sequential Gram-Schmidt against the earlier columns (not mutually orthogonal): with a_q = t.U_q of the incoming t
// and G = U'U, the coefficient of step q is c_q = (a_q - sum_{r<q} c_r G_rq) / G_qq; then t -= c_q U_q in that order
__global__ __launch_bounds__(256) void k_scca_gs(double *t, uint64_t P, const double *U, int j, const double *partA, int pstride, int nb,
                                                 const double *G, int ldg, double *partN, const int *flags)
{
   extern __shared__ double coef[]; // [j]
   __shared__ double red[4];
   if (flags[0]) return;
   for (int q = 0; q < j; q++) {
      const double a = sum_partials<4>(partA + 1 + q, nb, pstride, red);
      if (threadIdx.x == 0) coef[q] = a;
   }
   __syncthreads();
   if (threadIdx.x == 0)
      for (int q = 0; q < j; q++) {
         double a = coef[q];
         for (int r = 0; r < q; r++) a -= coef[r] * G[(size_t)r * ldg + q];
         coef[q] = a / G[(size_t)q * ldg + q];
      }
   __syncthreads();
   const uint64_t r = (uint64_t)blockIdx.x * RB + threadIdx.x;
   double x = 0;
   if (r < P) {
      x = t[r];
      for (int q = 0; q < j; q++) x -= coef[q] * U[(size_t)q * P + r];
      t[r] = x;
   }
   const double ss = block_sum<4>(x * x, red);
   if (threadIdx.x == 0) partN[blockIdx.x] = ss;
}

// first half of norm_thresh (randompca.cpp:233-239): t / ||t||, soft threshold; partial sums of the new squared norm
__global__ __launch_bounds__(256) void k_scca_thresh(double *t, uint64_t P, const double *partN, int nstride, int nb, double lambda,
                                                     double *partN2, const int *flags)
{
   __shared__ double red[4];
   if (flags[0]) return;
   const double s = sqrt(sum_partials<4>(partN, nb, nstride, red));
   const uint64_t r = (uint64_t)blockIdx.x * RB + threadIdx.x;
   double x = 0;
   if (r < P) {
      x = t[r];
      if (s > 0) {
         x /= s;
         const double z = fabs(x) - lambda;
         x = z < 0 ? 0.0 : (x > 0 ? z : (x < 0 ? -z : 0.0));
      }
      t[r] = x;
   }
   const double ss = block_sum<4>(x * x, red);
   if (threadIdx.x == 0) partN2[blockIdx.x] = ss;
}

// second half of norm_thresh: u = t / ||t|| (if > 0) into U[:, j], partM[blk] = {max |u - u_old|, max |u|}; then the workgroup's
// part of w = C'u, partW[blk][kp], rows with u = 0 skipped (after thresholding that is most of them)
__global__ __launch_bounds__(256) void k_scca_update(const double *t, uint64_t P, const double *partN2, int nb, const double *__restrict__ Cm,
                                                     int kp, double *Uj, double *partW, double *partM, const int *flags)
{
   __shared__ double ul[RB];
   __shared__ double wl[16][64];
   __shared__ double red[4];
   if (flags[0]) return;
   const double s = sqrt(sum_partials<4>(partN2, nb, 1, red));
   const uint64_t row0 = (uint64_t)blockIdx.x * RB, r = row0 + threadIdx.x;
   double u = 0, diff = 0;
   if (r < P) {
      u = t[r];
      if (s > 0) u /= s;
      diff = fabs(Uj[r] - u);
      Uj[r] = u;
   }
   ul[threadIdx.x] = u;
   const double dmax = block_max<4>(diff, red), umax = block_max<4>(fabs(u), red); // (the barriers inside also publish ul)
   if (threadIdx.x == 0) {
      partM[2 * (size_t)blockIdx.x] = dmax;
      partM[2 * (size_t)blockIdx.x + 1] = umax;
   }
   const int g = threadIdx.x >> 4, l = threadIdx.x & 15;
   for (int c0 = 0; c0 < kp; c0 += 64) {
      double acc[4] = {0, 0, 0, 0};
      for (int pass = 0; pass < RB / 16; pass++) {
         const double uu = ul[pass * 16 + g];
         if (uu != 0) { // (rows >= P hold 0)
            const double *row = Cm + (row0 + pass * 16 + g) * kp + c0 + l;
#pragma unroll
            for (int i = 0; i < 4; i++)
               if (c0 + l + 16 * i < kp) acc[i] += row[16 * i] * uu;
         }
      }
#pragma unroll
      for (int i = 0; i < 4; i++) wl[g][l + 16 * i] = acc[i];
      __syncthreads();
      if (threadIdx.x < 64 && c0 + (int)threadIdx.x < kp) {
         double w = 0;
         for (int gg = 0; gg < 16; gg++) w += wl[gg][threadIdx.x];
         partW[(size_t)blockIdx.x * kp + c0 + threadIdx.x] = w;
      }
      __syncthreads();
   }
}

// everything of length k, one workgroup: w = sum of the partial C'u; v <- w, the reference's Gram-Schmidt against V[:, <j]
// (randompca.cpp:470-478), norm_thresh(v, lambda2); the rule of :456-462 / :481-487 (all of u or v below tol: stop) and of :490-498
// (iter > 0 and both max-abs changes below tol: converged); d = u'C v = w.v for the v just made
template <int VT> __global__ __launch_bounds__(VT) void k_scca_v(const double *partW, const double *partM, int nb, int kp, int k, double *V, int j, double lambda2,
                                                double tol, int *flags, double *dcur)
{
   extern __shared__ double sh[]; // w [kp], v [kp]
   __shared__ double buf[VT];
   __shared__ double red[VT / 64];
   double *w = sh, *v = sh + kp;
   const int done = flags[0], iter = flags[1];
   __syncthreads();
   if (done) return;
   double m0 = 0, m1 = 0;
   for (int i = threadIdx.x; i < nb; i += VT) {
      m0 = fmax(m0, partM[2 * (size_t)i]);
      m1 = fmax(m1, partM[2 * (size_t)i + 1]);
   }
   const double du = block_max<VT / 64>(m0, red), umax = block_max<VT / 64>(m1, red);
   if (umax < tol) { // "U[j] is all zero, l1 penalty too large"
      if (threadIdx.x == 0) flags[0] = DONE_U_ZERO;
      return;
   }
   // w: cw columns at a time, the workgroups' partials dealt over ng groups of threads, the groups added in order
   const int cw = kp < VT ? kp : VT, ng = VT / cw, g = threadIdx.x / cw, cl = threadIdx.x % cw;
   for (int c0 = 0; c0 < kp; c0 += cw) {
      const int c = c0 + cl;
      double s = 0;
      if (g < ng && c < kp) { // (four independent chains: one workgroup reads all nb * kp partials, and it is the latency that costs)
         double s1 = 0, s2 = 0, s3 = 0;
         int b = g;
         for (; b + 3 * ng < nb; b += 4 * ng) {
            s += partW[(size_t)b * kp + c];
            s1 += partW[(size_t)(b + ng) * kp + c];
            s2 += partW[(size_t)(b + 2 * ng) * kp + c];
            s3 += partW[(size_t)(b + 3 * ng) * kp + c];
         }
         for (; b < nb; b += ng) s += partW[(size_t)b * kp + c];
         s = (s + s1) + (s2 + s3);
      }
      if (g < ng) buf[g * cw + cl] = s;
      __syncthreads();
      if (g == 0 && c < kp) {
         double tot = 0;
         for (int gg = 0; gg < ng; gg++) tot += buf[gg * cw + cl];
         w[c] = tot;
         v[c] = c < k ? tot : 0.0;
      }
      __syncthreads();
   }
   for (int q = 0; q < j; q++) {
      const double *Vq = V + (size_t)q * kp;
      double a = 0, n2 = 0;
      for (int c = threadIdx.x; c < k; c += VT) {
         a += v[c] * Vq[c];
         n2 += Vq[c] * Vq[c];
      }
      a = block_sum<VT / 64>(a, red);
      n2 = block_sum<VT / 64>(n2, red);
      for (int c = threadIdx.x; c < k; c += VT) v[c] -= a * Vq[c] / n2;
      __syncthreads();
   }
   double n2 = 0;
   for (int c = threadIdx.x; c < k; c += VT) n2 += v[c] * v[c];
   double s = sqrt(block_sum<VT / 64>(n2, red));
   if (s > 0) {
      n2 = 0;
      for (int c = threadIdx.x; c < k; c += VT) {
         double x = v[c] / s;
         const double z = fabs(x) - lambda2;
         x = z < 0 ? 0.0 : (x > 0 ? z : (x < 0 ? -z : 0.0));
         v[c] = x;
         n2 += x * x;
      }
      s = sqrt(block_sum<VT / 64>(n2, red));
   }
   double *Vj = V + (size_t)j * kp;
   double dv = 0, vmax = 0, dd = 0;
   for (int c = threadIdx.x; c < k; c += VT) {
      const double x = s > 0 ? v[c] / s : v[c];
      dv = fmax(dv, fabs(Vj[c] - x));
      vmax = fmax(vmax, fabs(x));
      dd += w[c] * x;
      Vj[c] = x;
   }
   dv = block_max<VT / 64>(dv, red);
   vmax = block_max<VT / 64>(vmax, red);
   dd = block_sum<VT / 64>(dd, red);
   if (threadIdx.x == 0) {
      dcur[0] = dd;
      if (vmax < tol)
         flags[0] = DONE_V_ZERO; // "V[j] is all zero, l2 penalty too large"
      else if (iter > 0 && dv < tol && du < tol)
         flags[0] = DONE_CONVERGED; // (flags[1] stays: the reference's `iter` at its break)
      else
         flags[1] = iter + 1;
   }
}

// a finished dimension's row and column of G = U'U: partG[blk][q] = sum over the workgroup's rows of U_q U_j, q <= j ...
__global__ __launch_bounds__(256) void k_scca_gram(const double *U, uint64_t P, int j, double *partG, int pstride)
{
   __shared__ double red[4];
   const uint64_t r = (uint64_t)blockIdx.x * RB + threadIdx.x;
   const double uj = r < P ? U[(size_t)j * P + r] : 0.0;
   for (int q = 0; q <= j; q++) {
      const double a = block_sum<4>(r < P ? uj * U[(size_t)q * P + r] : 0.0, red);
      if (threadIdx.x == 0) partG[(size_t)blockIdx.x * pstride + q] = a;
   }
}

// ... and their sum, one workgroup
__global__ __launch_bounds__(256) void k_scca_gram_sum(const double *partG, int pstride, int nb, int j, double *G, int ldg)
{
   __shared__ double red[4];
   for (int q = 0; q <= j; q++) {
      const double a = sum_partials<4>(partG + q, nb, pstride, red);
      if (threadIdx.x == 0) G[(size_t)q * ldg + j] = G[(size_t)j * ldg + q] = a;
   }
}

} // namespace

namespace fpca {

void scca_check_single(const fpca_ctx *c, const char *fn)
{
   if (c->multi() || (c->rank_known && c->nranks > 1))
      throw Error(FPCA_EINVAL, std::string(fn) + ": the context is one shard of several (a communicator, an all-reduce hook or fpca_set_rank with " +
                                   "more than one rank); SCCA normalises u over all SNPs and runs on a single context only");
   refuse_masked(c, fn);
}

void scca_store_c(const double *T, uint64_t P_g, int b, int nc, double scale, double *Cm, int kp, int c0, hipStream_t s)
{
   const uint64_t tot = P_g * (uint64_t)b;
   if (!tot) return;
   hipLaunchKernelGGL(k_scca_store_c, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, s, T, P_g, b, nc, scale, Cm, kp, c0);
   HIP_CHECK(hipGetLastError());
}

void scca_free(fpca_ctx *c)
{
   delete c->scca;
   c->scca = nullptr;
}

// randompca.cpp:402-415: standardise Y, scale by invdiv; then C = invdiv X'Yh instead of the operator
static void scca_prepare(fpca_ctx *c, const double *Y, int64_t ldy, int k, int stand_y, int divisor)
{
   const uint64_t N = c->N, P = c->P_g;
   HIP_CHECK(hipSetDevice(c->device));
   hipStream_t s = c->stream;
   HIP_CHECK(hipStreamSynchronize(s));
   scca_free(c); // (the next prepare replaces the first)
   ensure_stats(c);
   const int kp = pad16(k);
   auto st = std::make_unique<fpca_scca_state>();
   st->k = k;
   st->kp = kp;
   st->invdiv = divisor == FPCA_DIVISOR_N1 ? 1.0 / std::sqrt((double)N - 1.0) : 1.0;
   // (the state owns both, scca.hpp)
   st->d_C = static_cast<double *>(dev_alloc(std::max<size_t>((size_t)P * kp * sizeof(double), 8), "fpca_scca_prepare",
                                             ("the " + std::to_string(P) + " x " + std::to_string(k) + " cross-product matrix").c_str()));
   st->d_flags = static_cast<int *>(dev_alloc(16, "fpca_scca_prepare", "the iteration flags"));

   // phenotypes: rows of a [k][N_pad] image, standardised there (util.cpp:24-110), back as N x k, scaled
   st->Yh.resize((size_t)N * k);
   {
      DevMem<double> own((size_t)k * c->N_pad + 3 * (size_t)k, "fpca_scca_prepare", "the phenotypes");
      double *dY = own.p, *dstat = dY + (size_t)k * c->N_pad;
      HIP_CHECK(hipMemcpy2DAsync(dY, c->N_pad * sizeof(double), Y, (size_t)ldy * sizeof(double), N * sizeof(double), k, hipMemcpyHostToDevice, s));
      kern::dense_standardise(dY, c->N_pad, N, k, stand_y, dstat, dstat + k, dstat + 2 * k, s);
      HIP_CHECK(hipMemcpy2DAsync(st->Yh.data(), N * sizeof(double), dY, c->N_pad * sizeof(double), N * sizeof(double), k, hipMemcpyDeviceToHost, s));
      HIP_CHECK(hipStreamSynchronize(s));
   }
   if (st->invdiv != 1.0)
      for (double &y : st->Yh) y *= st->invdiv;

   // the chunked K2 pass X'Yh, each chunk copied into C's layout with the second invdiv
   ensure_io(c);
   for (int c0 = 0; c0 < k; c0 += MAX_BLOCKVEC) {
      const int nc = std::min(MAX_BLOCKVEC, k - c0), bw = pad16(nc);
      c->ensure(c->d_stage, c->stage_cap, (size_t)std::max(N, P) * nc);
      HIP_CHECK(hipMemcpyAsync(c->d_stage, st->Yh.data() + (size_t)c0 * N, (size_t)N * nc * sizeof(double), hipMemcpyHostToDevice, s));
      kern::colmajor_to_block(c->d_stage, N, N, c->N_pad, bw, nc, c->d_io_a, s);
      xt_dev(c, c->d_io_a, bw, s);
      scca_store_c(c->d_T, P, bw, nc, st->invdiv, st->d_C, kp, c0, s);
   }
   HIP_CHECK(hipStreamSynchronize(s));
   c->scca = st.release();
}

struct SccaOut {
   double *U;
   int64_t ldu;
   double *V;
   int64_t ldv;
   double *d, *Px;
   int64_t ldpx;
   double *Py;
   int64_t ldpy;
   int *converged, *iters;
   int64_t *nzero_x, *nzero_y;
   int *status;
};

void scca_fit_dev(fpca_ctx *c, fpca_scca_state *st, double lambda1, double lambda2, int ndim, int maxiter, double tol, const double *V0, int64_t ldv0,
                  SccaDevFit &fit)
{
   const uint64_t P = c->P_g;
   const int k = st->k, kp = st->kp;
   HIP_CHECK(hipSetDevice(c->device));
   hipStream_t s = c->stream;
   const int nb = (int)((P + RB - 1) / RB), ps = ndim + 1;

   // workspace: U [ndim][P] | t [P] | V [ndim][kp] | G [ndim][ndim] | partA [nb][ps] | partN, partN2 [nb] | partM [nb][2] | partW [nb][kp] | d
   const size_t oU = 0, ot = oU + (size_t)ndim * P, oV = ot + P, oG = oV + (size_t)ndim * kp, oA = oG + (size_t)ndim * ndim,
                oN = oA + (size_t)nb * ps, oN2 = oN + nb, oM = oN2 + nb, oW = oM + 2 * (size_t)nb, od = oW + (size_t)nb * kp, total = od + 2;
   if (total > st->ws_cap) {
      HIP_CHECK(hipStreamSynchronize(s));
      if (st->d_ws) (void)hipFree(st->d_ws);
      st->d_ws = nullptr;
      st->ws_cap = 0;
      st->d_ws = static_cast<double *>(dev_alloc(total * sizeof(double), "fpca_scca_fit / fpca_scca_cv", "the workspace of a fit")); // (the state's)
      st->ws_cap = total;
   }
   double *dU = st->d_ws + oU, *dt = st->d_ws + ot, *dV = st->d_ws + oV, *dG = st->d_ws + oG, *pA = st->d_ws + oA, *pN = st->d_ws + oN,
          *pN2 = st->d_ws + oN2, *pM = st->d_ws + oM, *pW = st->d_ws + oW, *dd = st->d_ws + od;
   int *flags = st->d_flags;
   HIP_CHECK(hipMemsetAsync(st->d_ws, 0, total * sizeof(double), s)); // U = 0 (randompca.cpp:423), V's pad rows, G
   HIP_CHECK(hipMemcpy2DAsync(dV, (size_t)kp * sizeof(double), V0, (size_t)ldv0 * sizeof(double), (size_t)k * sizeof(double), ndim, hipMemcpyHostToDevice, s));

   std::vector<double> d(ndim, 0.0);
   std::vector<int> iters(ndim, 0);
   int converged = 1, status = FPCA_SCCA_OK, jstop = ndim; // columns >= jstop were not finished
   const size_t lds_v = 2 * (size_t)kp * sizeof(double);
   for (int j = 0; j < ndim && converged; j++) {
      HIP_CHECK(hipMemsetAsync(flags, 0, 16, s));
      int h[2] = {0, 0};
      for (int it = 0; it < maxiter && !h[0];) {
         const int nbatch = std::min(BATCH, maxiter - it);
         for (int i = 0; i < nbatch; i++) {
            hipLaunchKernelGGL(k_scca_cv, dim3(nb), dim3(256), 0, s, st->d_C, P, kp, dV + (size_t)j * kp, dU, j, dt, pA, ps, flags);
            if (j > 0)
               hipLaunchKernelGGL(k_scca_gs, dim3(nb), dim3(256), (size_t)j * sizeof(double), s, dt, P, dU, j, pA, ps, nb, dG, ndim, pN, flags);
            hipLaunchKernelGGL(k_scca_thresh, dim3(nb), dim3(256), 0, s, dt, P, j > 0 ? pN : pA, j > 0 ? 1 : ps, nb, lambda1, pN2, flags);
            hipLaunchKernelGGL(k_scca_update, dim3(nb), dim3(256), 0, s, dt, P, pN2, nb, st->d_C, kp, dU + (size_t)j * P, pW, pM, flags);
            if (kp <= 64) // (the one workgroup reads all nb * kp partial sums: 16 waves hide that latency for a wide C, 4 are quicker through the barriers)
               hipLaunchKernelGGL(k_scca_v<256>, dim3(1), dim3(256), lds_v, s, pW, pM, nb, kp, k, dV, j, lambda2, tol, flags, dd);
            else
               hipLaunchKernelGGL(k_scca_v<1024>, dim3(1), dim3(1024), lds_v, s, pW, pM, nb, kp, k, dV, j, lambda2, tol, flags, dd);
         }
         HIP_CHECK(hipGetLastError());
         it += nbatch;
         HIP_CHECK(hipMemcpyAsync(h, flags, sizeof(h), hipMemcpyDeviceToHost, s));
         HIP_CHECK(hipStreamSynchronize(s));
      }
      iters[j] = h[1];
      if (h[0] == DONE_CONVERGED) {
         HIP_CHECK(hipMemcpyAsync(&d[j], dd, sizeof(double), hipMemcpyDeviceToHost, s));
         if (j + 1 < ndim) {
            hipLaunchKernelGGL(k_scca_gram, dim3(nb), dim3(256), 0, s, dU, P, j, pA, ps);
            hipLaunchKernelGGL(k_scca_gram_sum, dim3(1), dim3(256), 0, s, pA, ps, nb, j, dG, ndim);
            HIP_CHECK(hipGetLastError());
         }
         HIP_CHECK(hipStreamSynchronize(s));
         continue;
      }
      converged = 0;
      if (h[0] == 0) { // maxiter reached (randompca.cpp:501-507): the dimension's current u, v stay, d[j] = 0, nothing later is attempted
         status = FPCA_SCCA_MAXITER;
         jstop = j + 1;
      } else { // u or v vanished: this and the later columns are U = 0, V = V0, d = 0
         status = h[0] == DONE_U_ZERO ? FPCA_SCCA_LAMBDA1_TOO_LARGE : FPCA_SCCA_LAMBDA2_TOO_LARGE;
         jstop = j;
         HIP_CHECK(hipMemsetAsync(dU + (size_t)j * P, 0, P * sizeof(double), s));
      }
   }
   if (jstop < ndim) // V of the columns never finished: as given
      HIP_CHECK(hipMemcpy2DAsync(dV + (size_t)jstop * kp, (size_t)kp * sizeof(double), V0 + (size_t)jstop * ldv0, (size_t)ldv0 * sizeof(double),
                                 (size_t)k * sizeof(double), ndim - jstop, hipMemcpyHostToDevice, s));
   fit.dU = dU;
   fit.dV = dV;
   fit.d.swap(d);
   fit.iters.swap(iters);
   fit.converged = converged;
   fit.status = status;
}

static void scca_fit(fpca_ctx *c, double lambda1, double lambda2, int ndim, int maxiter, double tol, const double *V0, int64_t ldv0, const SccaOut &o)
{
   fpca_scca_state *st = c->scca;
   const uint64_t N = c->N, P = c->P_g;
   const int k = st->k, kp = st->kp;
   hipStream_t s = c->stream;
   SccaDevFit fit;
   scca_fit_dev(c, st, lambda1, lambda2, ndim, maxiter, tol, V0, ldv0, fit);
   const double *dU = fit.dU, *dV = fit.dV;
   const std::vector<double> &d = fit.d;
   const std::vector<int> &iters = fit.iters;
   const int converged = fit.converged, status = fit.status;

   // results.  U and V always come to the host: the non-zero counts and Py are host work
   std::vector<double> hV((size_t)k * ndim), hU_own;
   double *hU = o.U;
   int64_t ldu = o.ldu;
   if (!hU) {
      hU_own.resize((size_t)P * ndim);
      hU = hU_own.data();
      ldu = (int64_t)P;
   }
   HIP_CHECK(hipMemcpy2DAsync(hV.data(), (size_t)k * sizeof(double), dV, (size_t)kp * sizeof(double), (size_t)k * sizeof(double), ndim, hipMemcpyDeviceToHost, s));
   if (P) HIP_CHECK(hipMemcpy2DAsync(hU, (size_t)ldu * sizeof(double), dU, P * sizeof(double), P * sizeof(double), ndim, hipMemcpyDeviceToHost, s));
   HIP_CHECK(hipStreamSynchronize(s));
   for (int j = 0; j < ndim; j++) {
      if (o.V) std::memcpy(o.V + (size_t)j * o.ldv, hV.data() + (size_t)j * k, (size_t)k * sizeof(double));
      if (o.d) o.d[j] = d[j];
      if (o.iters) o.iters[j] = iters[j];
      if (o.nzero_x) { // randompca.cpp:509-510
         int64_t nz = 0;
         for (uint64_t i = 0; i < P; i++) nz += hU[(size_t)j * ldu + i] != 0;
         o.nzero_x[j] = nz;
      }
      if (o.nzero_y) {
         int64_t nz = 0;
         for (int i = 0; i < k; i++) nz += hV[(size_t)j * k + i] != 0;
         o.nzero_y[j] = nz;
      }
   }
   if (o.converged) *o.converged = converged;
   if (o.status) *o.status = status;
   if (o.Py) // Py = Yh V (randompca.cpp:527), in row blocks that stay in the host's cache across the k x ndim products
      for (uint64_t i0 = 0; i0 < N; i0 += 4096) {
         const uint64_t i1 = std::min<uint64_t>(N, i0 + 4096);
         for (int j = 0; j < ndim; j++) {
            double *py = o.Py + (size_t)j * o.ldpy;
            std::fill(py + i0, py + i1, 0.0);
            for (int q = 0; q < k; q++) {
               const double vq = hV[(size_t)j * k + q];
               if (vq == 0) continue;
               const double *y = st->Yh.data() + (size_t)q * N;
               for (uint64_t i = i0; i < i1; i++) py[i] += y[i] * vq;
            }
         }
      }
   if (o.Px) { // Px = invdiv X U (randompca.cpp:525-526): U in K3's operand layout, at most 64 columns at a time
      ensure_io(c);
      for (int c0 = 0; c0 < ndim; c0 += MAX_BLOCKVEC) {
         const int nc = std::min(MAX_BLOCKVEC, ndim - c0), bw = pad16(nc);
         c->ensure(c->d_stage, c->stage_cap, (size_t)std::max(N, P) * nc);
         c->ensure(c->d_T, c->T_cap, (size_t)c->P_pad * MAX_BLOCKVEC);
         kern::colmajor_to_t(dU + (size_t)c0 * P, P, P, c->P_pad, bw, nc, c->d_T, s);
         x_dev(c, bw, c->d_io_b, s);
         kern::block_to_colmajor(c->d_io_b, N, bw, nc, c->d_stage, N, s);
         staged_download(c, c->d_stage, N, nc, o.Px + (size_t)c0 * o.ldpx, o.ldpx, nullptr, 0, nullptr); // (synchronises)
      }
      if (st->invdiv != 1.0)
         for (int j = 0; j < ndim; j++)
            for (uint64_t i = 0; i < N; i++) o.Px[(size_t)j * o.ldpx + i] *= st->invdiv;
   }
}

} // namespace fpca

extern "C" int fpca_scca_prepare(fpca_ctx *ctx, const double *Y, int64_t ldy, int k, int stand_y, int divisor)
{
   return guarded([&] {
      if (!ctx || !Y) throw Error(FPCA_EINVAL, "bad argument to fpca_scca_prepare (NULL pointer)");
      scca_check_single(ctx, "fpca_scca_prepare");
      if (k < 1) throw Error(FPCA_EINVAL, "fpca_scca_prepare needs at least one phenotype (k >= 1)");
      if (k > SCCA_MAX_K)
         throw Error(FPCA_EINVAL, "fpca_scca_prepare: " + std::to_string(k) + " phenotypes; at most " + std::to_string(SCCA_MAX_K) +
                                      " are supported (the k-sized step keeps two vectors of that length in one workgroup's LDS: " +
                                      std::to_string(SCCA_V_LDS_MAX) + " B at the maximum, of the 160 KB gfx950 gives a workgroup)");
      if (ldy < (int64_t)ctx->N) throw Error(FPCA_EINVAL, "fpca_scca_prepare: ldy is smaller than the number of samples");
      if (stand_y < FPCA_STANDARDISE_NONE || stand_y > FPCA_STANDARDISE_CENTER)
         throw Error(FPCA_EINVAL, "fpca_scca_prepare: unknown phenotype standardisation " + std::to_string(stand_y));
      if (ctx->N < 2) throw Error(FPCA_EINVAL, "fpca_scca_prepare needs at least two samples");
      scca_prepare(ctx, Y, ldy, k, stand_y, divisor);
   });
}

extern "C" int fpca_debug_scca_lds(int device, int *max_k, int *need_at_max_k, int *per_workgroup)
{
   return guarded([&] {
      if (!max_k || !need_at_max_k || !per_workgroup) throw Error(FPCA_EINVAL, "bad argument to fpca_debug_scca_lds (NULL pointer)");
      *max_k = SCCA_MAX_K;
      *need_at_max_k = SCCA_V_LDS_MAX;
      HIP_CHECK(hipDeviceGetAttribute(per_workgroup, hipDeviceAttributeMaxSharedMemoryPerBlock, device));
   });
}

extern "C" int fpca_scca_fit(fpca_ctx *ctx, double lambda1, double lambda2, int ndim, int maxiter, double tol, const double *V0, int64_t ldv0,
                             double *U, int64_t ldu, double *V, int64_t ldv, double *d, double *Px, int64_t ldpx, double *Py, int64_t ldpy,
                             int *converged, int *iters, int64_t *nzero_x, int64_t *nzero_y, int *status)
{
   return guarded([&] {
      if (!ctx) throw Error(FPCA_EINVAL, "bad argument to fpca_scca_fit (NULL context)");
      scca_check_single(ctx, "fpca_scca_fit");
      if (!ctx->scca) throw Error(FPCA_EINVAL, "fpca_scca_fit: no phenotypes prepared (call fpca_scca_prepare on this context first)");
      const int k = ctx->scca->k;
      const uint64_t maxdim = std::min<uint64_t>(std::min<uint64_t>(ctx->N, ctx->P_g), (uint64_t)k);
      if (ndim < 1) throw Error(FPCA_EINVAL, "fpca_scca_fit: ndim can't be less than 1");
      if ((uint64_t)ndim > maxdim)
         throw Error(FPCA_EINVAL, "fpca_scca_fit: You asked for " + std::to_string(ndim) + " dimensions, but only " + std::to_string(maxdim) + " allowed");
      if (!(lambda1 >= 0)) throw Error(FPCA_EINVAL, "fpca_scca_fit: lambda1 must be non-negative");
      if (!(lambda2 >= 0)) throw Error(FPCA_EINVAL, "fpca_scca_fit: lambda2 must be non-negative");
      if (!(tol > 0)) throw Error(FPCA_EINVAL, "fpca_scca_fit: tol must be positive");
      if (maxiter < 1) throw Error(FPCA_EINVAL, "fpca_scca_fit: maxiter must be at least 1");
      if (!V0) throw Error(FPCA_EINVAL, "fpca_scca_fit: V0 (k x ndim starting vectors) is required");
      if (ldv0 < k) throw Error(FPCA_EINVAL, "fpca_scca_fit: ldv0 is smaller than the number of phenotypes");
      if (U && ldu < (int64_t)ctx->P_g) throw Error(FPCA_EINVAL, "fpca_scca_fit: ldu is smaller than the number of SNPs of the context");
      if (V && ldv < k) throw Error(FPCA_EINVAL, "fpca_scca_fit: ldv is smaller than the number of phenotypes");
      if (Px && ldpx < (int64_t)ctx->N) throw Error(FPCA_EINVAL, "fpca_scca_fit: ldpx is smaller than the number of samples");
      if (Py && ldpy < (int64_t)ctx->N) throw Error(FPCA_EINVAL, "fpca_scca_fit: ldpy is smaller than the number of samples");
      for (int j = 0; j < ndim; j++)
         for (int i = 0; i < k; i++)
            if (!std::isfinite(V0[(size_t)j * ldv0 + i])) throw Error(FPCA_EINVAL, "fpca_scca_fit: V0 holds a value that is not finite");
      scca_fit(ctx, lambda1, lambda2, ndim, maxiter, tol, V0, ldv0, SccaOut{U, ldu, V, ldv, d, Px, ldpx, Py, ldpy, converged, iters, nzero_x, nzero_y, status});
   });
}
