// pcrelate.hip -- PC-Relate (Conomos et al. 2016): kinship adjusted for the principal components, fpca_pcrelate_beta / fpca_pcrelate_block /
// fpca_pcrelate_tri (include/fpca.h "PC-Relate"), fpca_bench_pcrelate.
//
// Every SNP is regressed on V = [1 | pcs] over the training samples; the fitted value is an individual-specific allele frequency mu_is =
// V_i.beta_s / 2, and kin_ij = sum_s r_is r_js / (4 sum_s w_is w_js) with r = x - 2 mu, w = sqrt(mu (1 - mu)) at the usable (sample, SNP)
// cells and 0 elsewhere.  Two stages, each with an entry point of its own:
//   beta           B = V with the rows outside `train` zeroed goes through the context's K2 pass (xt_dev, one chunk: d <= 32 columns), T =
//                  X_g' B.  A = V_train' V_train and c = 1' V_train are formed (long double sums, rounded once) and A is factored (Cholesky,
//                  fp64) on the host before any device work; only L and c go to the device.  k_pcr_beta, one lane per SNP: rhs_sk = mean_s c_k
//                  + sd_s T_sk, then the two substitutions against L, staged in LDS beside one column per lane for its right-hand side.  beta
//                  stays on the device for the second stage; it is [P_g][d] row-major.
//   k_pcr_operands for a panel of C SNPs (a multiple of 512) and the samples a slab needs, r and w as ONE array of (r, w) pairs, each
//                  (sample, SNP) computed once.  Layout, in 16-byte (r, w) pairs: pair [(step * rows + p) * 16 + (snp ^ (p & 15))] for SNP
//                  `snp` of the 16-SNP step `step` and panel row p -- the 64 samples of a tile are 16 KB contiguous per step whatever sample
//                  the tile starts at, and the XOR is the LDS swizzle of the Gram kernel, applied here so that its copy is linear.  The
//                  codes come from a sample-major copy made for the call (kern::transpose_packed); beta of the block's 64 SNPs and V of its
//                  64 samples are staged in LDS (row stride 33: no bank conflict); the d-term dot product runs k = 0 .. d - 1.
//   k_pcr_gram     S = r r' and D = w w' together on v_mfma_f64_16x16x4_f64: k_grm_dot's geometry (a 2 x 2 wave workgroup per pair of
//                  64-sample tiles, a 32 x 32 block per wave, a triangle mode), eight accumulators (64 registers).  A step is 16 SNPs: the
//                  two tiles' 2 x 16 KB are loaded with 16-byte loads, linear, into registers under the previous step's MFMAs and stored to
//                  the other half of a 64 KB double buffer, one barrier per step; a lane then reads (r, w) of its sample with ONE
//                  ds_read_b128 (conflict-free by the swizzle) and every read feeds two products.  No atomics, no split along the SNPs:
//                  the accumulators live in the slab scratch between panels, the order of every sum is the SNP order.
//   k_pcr_finish   kin = S / (4 D): one exact multiply, ONE fp64 divide, D == 0 tested (NaN); the rectangle or the packed triangle rows.
// Slabs of rows as grm.hip: S and D of a slab within 256 MiB; per slab, per panel: operands, then Gram.  Panels within 1 GiB.
#include <algorithm>
#include <cmath>
#include <limits>

#include "ctx.hpp"
#include "launch_check.hpp"
#include "pcrelate.hpp"
#include "../../include/fpca_debug.h"

using namespace fpca;

namespace {

// lc: L [32][32] row-major (the lower triangle; what lies at or past d is the identity's and is not read), then c [32].  One lane per SNP; a
// lane's right-hand side lives in its own LDS column, so the loops over d index no register array.
__global__ __launch_bounds__(64) void k_pcr_beta(const double *__restrict__ T, int bw, const double *__restrict__ mean, const double *__restrict__ sd,
                                                  const double *__restrict__ lc, uint64_t P_g, int d, double *__restrict__ beta)
{
   __shared__ double L[PCR_MAXD * PCR_MAXD];
   __shared__ double cs[PCR_MAXD];
   __shared__ double ys[PCR_MAXD * 64];
   for (int e = threadIdx.x; e < PCR_MAXD * PCR_MAXD; e += 64) L[e] = lc[e];
   if (threadIdx.x < PCR_MAXD) cs[threadIdx.x] = lc[PCR_MAXD * PCR_MAXD + threadIdx.x];
   __syncthreads();
   const uint64_t s = (uint64_t)blockIdx.x * 64 + threadIdx.x;
   if (s >= P_g) return;
   const double mu = mean[s], sg = sd[s];
   double *b = beta + s * (uint64_t)d;
   if (!(sg > 1e-9 && mu == mu)) { // not live
      for (int k = 0; k < d; k++) b[k] = 0.0;
      return;
   }
   const double *t = T + s * (uint64_t)bw;
   double *y = ys + threadIdx.x;
   // L y' = rhs, rhs_k = mean c_k + sd T_k; then L' beta = y'
   for (int k = 0; k < d; k++) {
      double a = mu * cs[k] + sg * t[k];
      for (int j = 0; j < k; j++) a -= L[k * PCR_MAXD + j] * y[j * 64];
      y[k * 64] = a / L[k * PCR_MAXD + k];
   }
   for (int k = d - 1; k >= 0; k--) {
      double a = y[k * 64];
      for (int j = k + 1; j < d; j++) a -= L[j * PCR_MAXD + k] * y[j * 64];
      a /= L[k * PCR_MAXD + k];
      y[k * 64] = a;
      b[k] = a;
   }
}

// panel row p holds sample s0 + p for p < n0 and sample s1 + (p - n0) after that; samples at or past N give zeros.
// grid: x = the panel's 64-SNP groups (the first SNP of the panel is snp0), y = 64-row groups of the panel.
__global__ __launch_bounds__(256) void k_pcr_operands(const uint8_t *__restrict__ smp, size_t pitch, uint64_t N, const double *__restrict__ V,
                                                       const double *__restrict__ beta, const double *__restrict__ mean, const double *__restrict__ sd,
                                                       uint64_t P_g, int d, double lo, double hi, uint64_t snp0, uint64_t s0, uint64_t n0, uint64_t s1,
                                                       uint64_t rows, d2 *__restrict__ panel)
{
   __shared__ double bl[PCR_BLK_SNPS * (PCR_MAXD + 1)];
   __shared__ double vl[PCR_BLK_SNPS * (PCR_MAXD + 1)];
   __shared__ uint8_t lv[PCR_BLK_SNPS];
   const int tid = threadIdx.x;
   const uint64_t g0 = snp0 + (uint64_t)blockIdx.x * PCR_BLK_SNPS, p0 = (uint64_t)blockIdx.y * PCR_BLK_SNPS;
   for (int e = tid; e < PCR_BLK_SNPS * PCR_MAXD; e += 256) {
      const int a = e >> 5, k = e & 31;
      const uint64_t s = g0 + a, p = p0 + a, i = p < n0 ? s0 + p : s1 + (p - n0);
      bl[a * (PCR_MAXD + 1) + k] = (k < d && s < P_g) ? beta[s * (uint64_t)d + k] : 0.0;
      vl[a * (PCR_MAXD + 1) + k] = (k < d && p < rows && i < N) ? V[i * (uint64_t)d + k] : 0.0;
   }
   if (tid < PCR_BLK_SNPS) {
      const uint64_t s = g0 + tid;
      lv[tid] = s < P_g && sd[s] > 1e-9 && mean[s] == mean[s];
   }
   __syncthreads();
   const int t = tid & 15, ls = tid >> 4;
#pragma unroll 1
   for (int sg = 0; sg < 4; sg++) {
      const int a = sg * 16 + ls;
      const uint64_t p = p0 + a;
      if (p >= rows) continue;
      const uint64_t i = p < n0 ? s0 + p : s1 + (p - n0);
      const int sl = t ^ (int)(p & 15); // the SNP of the step whose pair this lane stores in slot t
      const double *vr = &vl[a * (PCR_MAXD + 1)];
#pragma unroll 1
      for (int st = 0; st < 4; st++) {
         const int sn = st * PCR_STEP + sl;
         const uint64_t s = g0 + sn;
         const uint32_t code = i < N ? (smp[i * pitch + (s >> 2)] >> (2 * (s & 3))) & 3u : 1u;
         const double *br = &bl[sn * (PCR_MAXD + 1)];
         double acc = 0.0;
         for (int k = 0; k < d; k++) acc = fma(vr[k], br[k], acc);
         const double mu = 0.5 * acc, x = code == 0 ? 2.0 : code == 2 ? 1.0 : 0.0;
         const bool usable = lv[sn] && code != 1u && mu > lo && mu < hi;
         d2 o;
         o.x = usable ? x - 2.0 * mu : 0.0;
         o.y = usable ? sqrt(mu * (1.0 - mu)) : 0.0;
         panel[(((uint64_t)blockIdx.x * 4 + st) * rows + p) * PCR_STEP + t] = o;
      }
   }
}

// workgroup w -> (tI, tJ) = (w / ntj, w % ntj): tile tI holds samples [i0 + 64 tI, ...) = panel rows pa0 + 64 tI ..., tile tJ samples
// [j0 + 64 tJ, ...) = panel rows pb0 + 64 tJ ...; every tile lies within the panel's `rows` rows.  S and D [(i - i0) * ld + (j - j0)] are
// read back unless this is the first panel.  TRI: blocks wholly above the diagonal are skipped.
template <bool TRI>
__global__ __launch_bounds__(256, 2) void k_pcr_gram(const d2 *__restrict__ panel, uint64_t rows, uint32_t nsteps, uint64_t pa0, uint64_t pb0, uint64_t i0,
                                                     uint64_t iend, uint64_t j0, uint64_t jend, uint32_t ntj, int first, double *__restrict__ S,
                                                     double *__restrict__ D, size_t ld)
{
   __shared__ d2 tile[2][2][PCR_TILE * PCR_STEP]; // [buffer][I, J][sample][slot]: 64 KB
   const uint64_t tI = blockIdx.x / ntj, tJ = blockIdx.x % ntj;
   if (TRI && j0 + tJ * PCR_TILE > i0 + tI * PCR_TILE + (PCR_TILE - 1)) return; // (uniform over the workgroup, before any barrier)
   const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, m = lane & 15, k = lane >> 4, wr = wave >> 1, wc = wave & 1;
   const uint64_t ia = i0 + tI * PCR_TILE + (uint64_t)wr * 32, ja = j0 + tJ * PCR_TILE + (uint64_t)wc * 32;
   const bool active = ia < iend && ja < jend && !(TRI && ja > ia + 31); // a wave without work still stages the tiles and meets the barriers
   const uint64_t pI = pa0 + tI * PCR_TILE, pJ = pb0 + tJ * PCR_TILE;
   const d2 *srcI = panel + pI * PCR_STEP + tid, *srcJ = panel + pJ * PCR_STEP + tid;
   const size_t stride = (size_t)rows * PCR_STEP;
   d4 aS[2][2], aD[2][2];
#pragma unroll
   for (int a = 0; a < 2; a++)
#pragma unroll
      for (int b = 0; b < 2; b++) {
         aS[a][b] = d4{0.0, 0.0, 0.0, 0.0};
         aD[a][b] = d4{0.0, 0.0, 0.0, 0.0};
         const uint64_t j = ja + 16 * b + m;
         if (first || !active || j >= jend) continue;
#pragma unroll
         for (int r = 0; r < 4; r++) {
            const uint64_t i = ia + 16 * a + k + 4 * r;
            if (i < iend) {
               aS[a][b][r] = S[(size_t)(i - i0) * ld + (j - j0)];
               aD[a][b][r] = D[(size_t)(i - i0) * ld + (j - j0)];
            }
         }
      }
   auto fetch = [&](uint32_t st, d2 (&t)[8]) {
#pragma unroll
      for (int u = 0; u < 4; u++) {
         t[u] = srcI[(size_t)st * stride + 256 * u];
         t[4 + u] = srcJ[(size_t)st * stride + 256 * u];
      }
   };
   auto stage = [&](int buf, const d2 (&t)[8]) {
#pragma unroll
      for (int u = 0; u < 4; u++) {
         tile[buf][0][tid + 256 * u] = t[u];
         tile[buf][1][tid + 256 * u] = t[4 + u];
      }
   };
   {
      d2 t[8];
      fetch(0, t);
      stage(0, t);
   }
   __syncthreads();
   // the pair of SNP `snp` of panel row p is in slot snp ^ (p & 15); rows 16 apart share the swizzle
   const int swA = (int)((pI + wr * 32 + m) & 15), swB = (int)((pJ + wc * 32 + m) & 15);
   for (uint32_t st = 0; st < nsteps; st++) {
      const int buf = st & 1;
      const bool more = st + 1 < nsteps;
      d2 nxt[8];
      if (more) fetch(st + 1, nxt);
      if (active) {
         const d2 *tA = &tile[buf][0][(wr * 32 + m) * PCR_STEP], *tB = &tile[buf][1][(wc * 32 + m) * PCR_STEP];
#pragma unroll
         for (int q = 0; q < 4; q++) {
            const int snp = 4 * q + k;
            const d2 a0 = tA[snp ^ swA], a1 = tA[16 * PCR_STEP + (snp ^ swA)], b0 = tB[snp ^ swB], b1 = tB[16 * PCR_STEP + (snp ^ swB)];
            aS[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0.x, b0.x, aS[0][0], 0, 0, 0);
            aD[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0.y, b0.y, aD[0][0], 0, 0, 0);
            aS[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0.x, b1.x, aS[0][1], 0, 0, 0);
            aD[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0.y, b1.y, aD[0][1], 0, 0, 0);
            aS[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1.x, b0.x, aS[1][0], 0, 0, 0);
            aD[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1.y, b0.y, aD[1][0], 0, 0, 0);
            aS[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1.x, b1.x, aS[1][1], 0, 0, 0);
            aD[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1.y, b1.y, aD[1][1], 0, 0, 0);
         }
      }
      // every wave has read buffer buf ^ 1 before the barrier that ended the previous step
      if (more) stage(buf ^ 1, nxt);
      __syncthreads();
   }
   if (!active) return;
   // v_mfma_f64_16x16x4_f64: register r of lane (m, k) is D[row = k + 4 r][col = m]
#pragma unroll
   for (int a = 0; a < 2; a++)
#pragma unroll
      for (int b = 0; b < 2; b++) {
         const uint64_t j = ja + 16 * b + m;
         if (j >= jend) continue;
#pragma unroll
         for (int r = 0; r < 4; r++) {
            const uint64_t i = ia + 16 * a + k + 4 * r;
            if (i < iend) {
               S[(size_t)(i - i0) * ld + (j - j0)] = aS[a][b][r];
               D[(size_t)(i - i0) * ld + (j - j0)] = aD[a][b][r];
            }
         }
      }
}

// one thread per cell (a, b) of the slab: sample i = i0 + a (row), column b.  RECT: kin[a * ld + b]; TRI: the columns start at sample 0,
// kin[i (i + 1) / 2 + b - i0 (i0 + 1) / 2] for b <= i.  den (may be null) likewise.
template <int MODE>
__global__ __launch_bounds__(256) void k_pcr_finish(const double *__restrict__ S, const double *__restrict__ D, size_t ld, uint64_t i0, uint64_t ni,
                                                     uint64_t nj, double *__restrict__ kin, double *__restrict__ den)
{
   const uint64_t b = (uint64_t)blockIdx.x * 256 + threadIdx.x, a = blockIdx.y;
   if (b >= nj || a >= ni) return;
   const uint64_t i = i0 + a;
   if (MODE == PCR_TRI && b > i) return;
   const size_t at = (size_t)a * ld + b;
   const double dd = D[at];
   const double v = dd == 0.0 ? __builtin_nan("") : S[at] / (4.0 * dd);
   const size_t o = MODE == PCR_RECT ? at : (size_t)(i * (i + 1) / 2 - i0 * (i0 + 1) / 2 + b);
   kin[o] = v;
   if (den) den[o] = dd;
}

} // namespace

// ---- host: what pcrelate_ibd.hip shares is declared in pcrelate.hpp ------------------------------------------------------

namespace fpca {

void pcr_refuse(const fpca_ctx *c, const char *fn)
{
   if (!c) throw Error(FPCA_EINVAL, std::string("bad argument to ") + fn + " (NULL context)");
   if (c->dense)
      throw Error(FPCA_EINVAL, std::string(fn) + ": this context holds a dense matrix; PC-Relate is computed from the packed genotypes "
                                                 "(fpca_create, fpca_create_from_bed, synthetic)");
   if (c->masked())
      throw Error(FPCA_EINVAL, std::string(fn) + ": a sample mask is set (fpca_set_sample_mask); clear it (the training samples are passed as `train`)");
   if (c->multi() || (c->rank_known && c->nranks > 1))
      throw Error(FPCA_EINVAL, std::string(fn) + ": this context is one shard of several (a communicator, an all-reduce hook or fpca_set_rank with "
                                                 "more than one rank); PC-Relate sums over all SNPs -- compute it on a single context");
   if (c->P_g == 0) throw Error(FPCA_EINVAL, std::string(fn) + ": this context has no SNPs");
   if (c->N > 0xFFFFFFFFull) throw Error(FPCA_EINVAL, std::string(fn) + ": this context has " + std::to_string(c->N) + " samples; at most 2^32 - 1");
}

// V = [1 | pcs], N x d row-major
std::vector<double> pcr_design(const fpca_ctx *c, const char *fn, const double *pcs, int npc)
{
   if (npc < 0 || npc > PCR_MAXD - 1)
      throw Error(FPCA_EINVAL, std::string(fn) + ": npc = " + std::to_string(npc) + " is outside 0 .. " + std::to_string(PCR_MAXD - 1));
   if (npc > 0 && !pcs) throw Error(FPCA_EINVAL, std::string("bad argument to ") + fn + " (pcs is NULL)");
   const uint64_t N = c->N;
   const int d = npc + 1;
   std::vector<double> V((size_t)N * d);
   for (uint64_t i = 0; i < N; i++) {
      V[(size_t)i * d] = 1.0;
      for (int k = 0; k < npc; k++) {
         const double v = pcs[(size_t)i * npc + k];
         if (!std::isfinite(v))
            throw Error(FPCA_EINVAL, std::string(fn) + ": pcs[" + std::to_string(i) + "][" + std::to_string(k) + "] is not finite");
         V[(size_t)i * d + 1 + k] = v;
      }
   }
   return V;
}

// A = V_train' V_train and c = 1' V_train in long double, rounded once; L L' = A in fp64.  lc: L padded to 32 x 32 with the identity, then c.
void pcr_factor(const fpca_ctx *c, const char *fn, const std::vector<double> &V, int d, const uint8_t *train, std::vector<double> &lc)
{
   const uint64_t N = c->N;
   uint64_t nt = 0;
   std::vector<long double> A((size_t)d * d, 0.0L), cs(d, 0.0L);
   for (uint64_t i = 0; i < N; i++) {
      if (train && !train[i]) continue;
      nt++;
      const double *v = &V[(size_t)i * d];
      for (int a = 0; a < d; a++) {
         cs[a] += v[a];
         for (int b = 0; b <= a; b++) A[(size_t)a * d + b] += (long double)v[a] * v[b];
      }
   }
   if (nt < (uint64_t)d + 1)
      throw Error(FPCA_EINVAL, std::string(fn) + ": " + std::to_string(nt) + " training samples; a regression on " + std::to_string(d) +
                                   " columns needs at least " + std::to_string(d + 1));
   lc.assign((size_t)PCR_MAXD * PCR_MAXD + PCR_MAXD, 0.0);
   for (int k = 0; k < PCR_MAXD; k++) lc[(size_t)k * PCR_MAXD + k] = 1.0;
   double *L = lc.data();
   double pmax = 0.0;
   for (int k = 0; k < d; k++) {
      for (int j = 0; j <= k; j++) {
         double a = (double)A[(size_t)k * d + j];
         for (int q = 0; q < j; q++) a -= L[k * PCR_MAXD + q] * L[j * PCR_MAXD + q];
         if (j < k) {
            L[k * PCR_MAXD + j] = a / L[j * PCR_MAXD + j];
         } else {
            pmax = std::max(pmax, a);
            if (!(a > 1e-12 * pmax))
               throw Error(FPCA_EINVAL, std::string(fn) + ": [1 | pcs] is rank deficient over the training samples (column " + std::to_string(k) +
                                            " is a linear combination of the ones before it: pivot " + std::to_string(a) + " against " + std::to_string(pmax) + ")");
            L[k * PCR_MAXD + k] = std::sqrt(a);
         }
      }
      lc[(size_t)PCR_MAXD * PCR_MAXD + k] = (double)cs[k];
   }
}

// beta on the device from the factor: the K2 pass of B = V with the rows outside train zeroed, then the solve
void pcr_beta_dev(fpca_ctx *c, const char *fn, const std::vector<double> &V, int d, const uint8_t *train, const std::vector<double> &lc, double *d_beta)
{
   const uint64_t N = c->N;
   hipStream_t s = c->stream;
   ensure_stats(c);
   ensure_io(c);
   const int bw = pad16(d); // d <= 32: one chunk of the K2 pass
   std::vector<double> B((size_t)c->N_pad * bw, 0.0);
   for (uint64_t i = 0; i < N; i++)
      if (!train || train[i])
         for (int k = 0; k < d; k++) B[(size_t)i * bw + k] = V[(size_t)i * d + k];
   DevMem<double> d_lc(lc.size(), fn, "the Cholesky factor");
   HIP_CHECK(hipMemcpyAsync(c->d_io_a, B.data(), B.size() * sizeof(double), hipMemcpyHostToDevice, s));
   HIP_CHECK(hipMemcpyAsync(d_lc.p, lc.data(), lc.size() * sizeof(double), hipMemcpyHostToDevice, s));
   xt_dev(c, c->d_io_a, bw, s);
   hipLaunchKernelGGL(k_pcr_beta, dim3((unsigned)((c->P_g + 63) / 64)), dim3(64), 0, s, c->d_T, bw, c->d_mean, c->d_sd, d_lc.p, c->P_g, d, d_beta);
   launch_check();
   HIP_CHECK(hipStreamSynchronize(s)); // (B and lc are the host's)
}

uint64_t pcr_env(const char *v, uint64_t unit)
{
   if (!v || std::atoll(v) <= 0) return 0;
   return round_up((uint64_t)std::atoll(v), unit);
}

// rows of a slab whose cells are `cols` wide: S and D within PCR_SLAB_BYTES, the tile pairs within one launch; whole tiles, at least one
} // namespace fpca

namespace {

uint64_t pcr_slab_rows(uint64_t cols)
{
   if (const uint64_t forced = PCR_ENV("FPCA_PCR_SLAB_ROWS", PCR_TILE)) return forced;
   const uint64_t by_mem = PCR_SLAB_BYTES / (cols * 2 * sizeof(double)) / PCR_TILE;
   const uint64_t by_launch = PCR_LAUNCH_PAIRS / ((cols + PCR_TILE - 1) / PCR_TILE);
   return std::min<uint64_t>(std::max<uint64_t>(std::min(by_mem, by_launch), 1), 512) * PCR_TILE; // (a row is one grid.y of k_pcr_finish)
}

} // namespace

namespace fpca {

// the sample-major copy, V and (given) beta on the device
void pcr_make_operand(fpca_ctx *c, PcrBufs &s, const char *fn, const std::vector<double> &V, int d, const double *beta)
{
   ensure_stats(c);
   s.d = d;
   s.pitch = (size_t)round_up(c->P_pad / 4, 128);
   const size_t need = (size_t)c->N_pad * s.pitch;
   char detail[96];
   std::snprintf(detail, sizeof(detail), "%llu samples x %llu bytes", (unsigned long long)c->N_pad, (unsigned long long)s.pitch);
   s.d_smp = DevMem<uint8_t>(need, fn, "sample-major copy", 0, detail, c->device);
   HIP_CHECK(hipMemsetAsync(s.d_smp.p, PAD_BYTE, need, c->stream));
   kern::transpose_packed(c->d_packed, c->pitch, c->N_pad, c->P_pad, s.d_smp.p, s.pitch, c->stream, false);
   s.d_V = DevMem<double>(V.size(), fn, "the design matrix [1 | pcs]");
   HIP_CHECK(hipMemcpyAsync(s.d_V.p, V.data(), V.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
   s.d_beta = DevMem<double>((size_t)c->P_g * d, fn, "the regression coefficients");
   if (beta) HIP_CHECK(hipMemcpyAsync(s.d_beta.p, beta, (size_t)c->P_g * d * sizeof(double), hipMemcpyHostToDevice, c->stream));
}

} // namespace fpca

namespace {

// the panel for slabs that need up to `rows` panel rows: as many whole chunks as PCR_PANEL_BYTES holds, at least one
void pcr_alloc_panel(const fpca_ctx *c, PcrBufs &s, uint64_t rows, const char *fn)
{
   const uint64_t slots = round_up(c->P_g, PCR_CHUNK);
   uint64_t snps = PCR_ENV("FPCA_PCR_PANEL_SNPS", PCR_CHUNK);
   if (!snps) snps = PCR_PANEL_BYTES / (rows * sizeof(d2)) / PCR_CHUNK * PCR_CHUNK;
   if (!snps)
      throw Error(FPCA_ENOMEM, std::string(fn) + ": one panel of " + std::to_string(PCR_CHUNK) + " SNPs x " + std::to_string(rows) + " samples needs " +
                                   std::to_string(rows * sizeof(d2) * PCR_CHUNK) + " bytes, the panels are capped at " + std::to_string(PCR_PANEL_BYTES) +
                                   "; call fpca_pcrelate_block on fewer samples at a time");
   s.panel_snps = std::min(snps, slots);
   s.panel_rows = rows;
   char detail[128];
   std::snprintf(detail, sizeof(detail), "r and w of %llu SNPs x %llu samples", (unsigned long long)s.panel_snps, (unsigned long long)rows);
   s.d_panel = DevMem<d2>((size_t)s.panel_snps * rows, fn, "operand panel", 0, detail, c->device);
}

void pcr_alloc_slab(const fpca_ctx *c, PcrBufs &s, uint64_t rows, uint64_t cols, bool out, bool den, const char *fn)
{
   s.ld = (size_t)cols;
   const size_t cells = (size_t)rows * cols;
   char detail[128];
   std::snprintf(detail, sizeof(detail), "a slab of %llu rows x %llu samples", (unsigned long long)rows, (unsigned long long)cols);
   s.d_S = DevMem<double>(cells, fn, "slab scratch (numerators)", 0, detail, c->device);
   s.d_D = DevMem<double>(cells, fn, "slab scratch (denominators)", 0, detail, c->device);
   if (out) s.d_kin = DevMem<double>(cells, fn, "slab scratch (output)", 0, detail, c->device);
   if (out && den) s.d_den = DevMem<double>(cells, fn, "slab scratch (output denominators)", 0, detail, c->device);
}

} // namespace

namespace fpca {

PcrMap pcr_map(uint64_t i0, uint64_t iend, uint64_t j0, uint64_t jend)
{
   const uint64_t ea = i0 + round_up(iend - i0, PCR_TILE), eb = j0 + round_up(jend - j0, PCR_TILE);
   if (std::max(i0, j0) <= std::min(ea, eb)) {
      const uint64_t lo = std::min(i0, j0), hi = std::max(ea, eb);
      return {lo, hi - lo, 0, hi - lo, i0 - lo, j0 - lo};
   }
   return {i0, ea - i0, j0, (ea - i0) + (eb - j0), 0, ea - i0};
}

} // namespace fpca

namespace {

// S and D of the cells [i0, iend) x [j0, jend) into the slab scratch: per panel, the operands, then the Gram.  what: 3 both kernels, 1 the
// operand kernel alone, 2 the Gram alone (on whatever the panel holds: the bench hook)
void pcr_products(const fpca_ctx *c, const PcrBufs &s, bool tri, uint64_t i0, uint64_t iend, uint64_t j0, uint64_t jend, int what = 3)
{
   const uint64_t nti = (iend - i0 + PCR_TILE - 1) / PCR_TILE, ntj = (jend - j0 + PCR_TILE - 1) / PCR_TILE, wgs = nti * ntj;
   if (!wgs) return;
   if (wgs > 0x7FFFFFFFull || ntj > 0xFFFFFFFFull) throw Error(FPCA_EINVAL, "PC-Relate: " + std::to_string(wgs) + " tile pairs exceed one launch");
   const PcrMap mp = pcr_map(i0, iend, j0, jend);
   if (mp.rows > s.panel_rows) throw Error(FPCA_EHIP, "PC-Relate: a slab needs more panel rows than were allocated");
   const uint64_t slots = round_up(c->P_g, PCR_CHUNK);
   for (uint64_t snp0 = 0; snp0 < slots; snp0 += s.panel_snps) {
      const uint64_t cc = std::min(s.panel_snps, slots - snp0);
      if (what & 1) {
         hipLaunchKernelGGL(k_pcr_operands, dim3((unsigned)(cc / PCR_BLK_SNPS), (unsigned)((mp.rows + PCR_BLK_SNPS - 1) / PCR_BLK_SNPS)), dim3(256), 0,
                            c->stream, s.d_smp.p, s.pitch, c->N, s.d_V.p, s.d_beta.p, c->d_mean, c->d_sd, c->P_g, s.d, s.lo, s.hi, snp0, mp.s0, mp.n0, mp.s1,
                            mp.rows, s.d_panel.p);
         launch_check();
      }
      if (what & 2) {
         if (tri)
            hipLaunchKernelGGL(k_pcr_gram<true>, dim3((unsigned)wgs), dim3(256), 0, c->stream, s.d_panel.p, mp.rows, (uint32_t)(cc / PCR_STEP), mp.pa0, mp.pb0,
                               i0, iend, j0, jend, (uint32_t)ntj, (int)(snp0 == 0), s.d_S.p, s.d_D.p, s.ld);
         else
            hipLaunchKernelGGL(k_pcr_gram<false>, dim3((unsigned)wgs), dim3(256), 0, c->stream, s.d_panel.p, mp.rows, (uint32_t)(cc / PCR_STEP), mp.pa0, mp.pb0,
                               i0, iend, j0, jend, (uint32_t)ntj, (int)(snp0 == 0), s.d_S.p, s.d_D.p, s.ld);
         launch_check();
      }
   }
}

void pcr_finish(int mode, const fpca_ctx *c, const PcrBufs &s, uint64_t i0, uint64_t ni, uint64_t nj)
{
   const dim3 grid((unsigned)((nj + 255) / 256), (unsigned)ni), block(256);
   if (mode == PCR_RECT)
      hipLaunchKernelGGL(k_pcr_finish<PCR_RECT>, grid, block, 0, c->stream, s.d_S.p, s.d_D.p, s.ld, i0, ni, nj, s.d_kin.p, s.d_den.p);
   else
      hipLaunchKernelGGL(k_pcr_finish<PCR_TRI>, grid, block, 0, c->stream, s.d_S.p, s.d_D.p, s.ld, i0, ni, nj, s.d_kin.p, s.d_den.p);
   launch_check();
}

uint64_t pcr_tri_rows(uint64_t N) { return std::min<uint64_t>(pcr_slab_rows(N), round_up(N, PCR_TILE)); }

// what fpca_pcrelate_block and fpca_pcrelate_tri share.  Everything up to pcr_make_operand is host work: every refusal comes first.
void pcr_run(fpca_ctx *ctx, const char *fn, int mode, const double *pcs, int npc, const double *beta, const uint8_t *train, double eps, uint64_t i0,
             uint64_t ni, uint64_t j0, uint64_t nj, double *kin, double *den)
{
   pcr_refuse(ctx, fn);
   if (!kin) throw Error(FPCA_EINVAL, std::string("bad argument to ") + fn + " (kin is NULL)");
   const uint64_t N = ctx->N;
   if (mode == PCR_RECT) {
      if (ni == 0 || nj == 0 || i0 >= N || ni > N - i0 || j0 >= N || nj > N - j0)
         throw Error(FPCA_EINVAL, std::string(fn) + ": samples [" + std::to_string(i0) + ", " + std::to_string(i0) + " + " + std::to_string(ni) + ") x [" +
                                      std::to_string(j0) + ", " + std::to_string(j0) + " + " + std::to_string(nj) +
                                      ") are not a non-empty rectangle of this context's " + std::to_string(N) + " samples");
      if (ni > PCR_BLOCK_LIMIT / sizeof(double) / nj)
         throw Error(FPCA_EINVAL, std::string(fn) + ": a block of " + std::to_string(ni) + " x " + std::to_string(nj) + " doubles is over the limit of " +
                                      std::to_string(PCR_BLOCK_LIMIT) + " bytes; call it block by block");
   }
   if (!(eps >= 0.0 && eps < 0.5)) throw Error(FPCA_EINVAL, std::string(fn) + ": eps = " + std::to_string(eps) + " is outside 0 <= eps < 0.5");
   const std::vector<double> V = pcr_design(ctx, fn, pcs, npc);
   const int d = npc + 1;
   std::vector<double> lc;
   if (beta) {
      for (size_t e = 0; e < (size_t)ctx->P_g * d; e++)
         if (!std::isfinite(beta[e]))
            throw Error(FPCA_EINVAL, std::string(fn) + ": beta[" + std::to_string(e / d) + "][" + std::to_string(e % d) + "] is not finite");
   } else {
      pcr_factor(ctx, fn, V, d, train, lc);
   }
   HIP_CHECK(hipSetDevice(ctx->device));
   PcrBufs s;
   s.lo = eps;
   s.hi = 1.0 - eps;
   pcr_make_operand(ctx, s, fn, V, d, beta);
   if (!beta) pcr_beta_dev(ctx, fn, V, d, train, lc, s.d_beta.p);
   if (mode == PCR_RECT) {
      const uint64_t rows = std::min<uint64_t>(pcr_slab_rows(nj), round_up(ni, PCR_TILE));
      pcr_alloc_panel(ctx, s, rows + round_up(nj, PCR_TILE), fn);
      pcr_alloc_slab(ctx, s, rows, nj, true, den != nullptr, fn);
      for (uint64_t a = i0; a < i0 + ni; a += rows) {
         const uint64_t b = std::min(a + rows, i0 + ni);
         const size_t cells = (size_t)(b - a) * nj, at = (size_t)(a - i0) * nj;
         pcr_products(ctx, s, false, a, b, j0, j0 + nj);
         pcr_finish(PCR_RECT, ctx, s, a, b - a, nj);
         HIP_CHECK(hipMemcpyAsync(kin + at, s.d_kin.p, cells * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
         if (den) HIP_CHECK(hipMemcpyAsync(den + at, s.d_den.p, cells * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
      }
   } else {
      const uint64_t rows = pcr_tri_rows(N);
      pcr_alloc_panel(ctx, s, round_up(N, PCR_TILE), fn);
      pcr_alloc_slab(ctx, s, rows, N, true, den != nullptr, fn);
      for (uint64_t a = 0; a < N; a += rows) {
         const uint64_t b = std::min(a + rows, N);
         const size_t at = (size_t)(a * (a + 1) / 2), cells = (size_t)(b * (b + 1) / 2) - at; // the packed rows a .. b - 1
         pcr_products(ctx, s, true, a, b, 0, b);
         pcr_finish(PCR_TRI, ctx, s, a, b - a, b);
         // the slab goes to the host as it finishes; the next one's kernels queue behind the copy
         HIP_CHECK(hipMemcpyAsync(kin + at, s.d_kin.p, cells * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
         if (den) HIP_CHECK(hipMemcpyAsync(den + at, s.d_den.p, cells * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
      }
   }
   HIP_CHECK(hipStreamSynchronize(ctx->stream));
}

} // namespace

extern "C" int fpca_pcrelate_beta(fpca_ctx *ctx, const double *pcs, int npc, const uint8_t *train, double *beta)
{
   return guarded([&] {
      const char *fn = "fpca_pcrelate_beta";
      pcr_refuse(ctx, fn);
      if (!beta) throw Error(FPCA_EINVAL, "bad argument to fpca_pcrelate_beta (beta is NULL)");
      const std::vector<double> V = pcr_design(ctx, fn, pcs, npc);
      const int d = npc + 1;
      std::vector<double> lc;
      pcr_factor(ctx, fn, V, d, train, lc);
      HIP_CHECK(hipSetDevice(ctx->device));
      DevMem<double> d_beta((size_t)ctx->P_g * d, fn, "the regression coefficients");
      pcr_beta_dev(ctx, fn, V, d, train, lc, d_beta.p);
      HIP_CHECK(hipMemcpy(beta, d_beta.p, (size_t)ctx->P_g * d * sizeof(double), hipMemcpyDeviceToHost));
   });
}

extern "C" int fpca_pcrelate_block(fpca_ctx *ctx, const double *pcs, int npc, const double *beta, const uint8_t *train, double eps, uint64_t i0,
                                   uint64_t ni, uint64_t j0, uint64_t nj, double *kin, double *den)
{
   return guarded([&] { pcr_run(ctx, "fpca_pcrelate_block", PCR_RECT, pcs, npc, beta, train, eps, i0, ni, j0, nj, kin, den); });
}

extern "C" int fpca_pcrelate_tri(fpca_ctx *ctx, const double *pcs, int npc, const double *beta, const uint8_t *train, double eps, double *kin, double *den)
{
   return guarded([&] { pcr_run(ctx, "fpca_pcrelate_tri", PCR_TRI, pcs, npc, beta, train, eps, 0, 0, 0, 0, kin, den); });
}

extern "C" int fpca_bench_pcrelate(fpca_ctx *ctx, int npc, int reps, double *ms, double *flops)
{
   return guarded([&] {
      const char *fn = "fpca_bench_pcrelate";
      pcr_refuse(ctx, fn);
      if (!ms || reps < 1 || npc < 0 || npc > PCR_MAXD - 1) throw Error(FPCA_EINVAL, "bad argument to fpca_bench_pcrelate");
      HIP_CHECK(hipSetDevice(ctx->device));
      const uint64_t N = ctx->N, P = ctx->P_g;
      const int d = npc + 1;
      // a model that leaves every called entry of a live SNP usable: mu = 0.5 + 0.01 sum_k V_ik, |V_ik| <= 1 / npc
      std::vector<double> V((size_t)N * d), beta((size_t)P * d);
      for (uint64_t i = 0; i < N; i++) {
         V[(size_t)i * d] = 1.0;
         for (int k = 1; k < d; k++) V[(size_t)i * d + k] = (double)((int)((i * 7 + k * 13) % 21) - 10) / (10.0 * npc);
      }
      for (uint64_t j = 0; j < P; j++) {
         beta[(size_t)j * d] = 1.0;
         for (int k = 1; k < d; k++) beta[(size_t)j * d + k] = 0.02;
      }
      PcrBufs s;
      s.lo = 0.01;
      s.hi = 0.99;
      pcr_make_operand(ctx, s, fn, V, d, beta.data());
      const uint64_t rows = pcr_tri_rows(N);
      pcr_alloc_panel(ctx, s, round_up(N, PCR_TILE), fn);
      pcr_alloc_slab(ctx, s, rows, N, false, false, fn);
      // the Gram kernel alone over the whole triangle, slab by slab and panel by panel as fpca_pcrelate_tri launches it, on the panel the
      // untimed pass left (test build, FPCA_PCR_BENCH_OPERANDS=1: the operand kernel alone instead)
      const char *v = FPCA_TEST_ENV("FPCA_PCR_BENCH_OPERANDS");
      const int what = (v && *v && *v != '0') ? 1 : 2;
      DevEvent e0(fn), e1(fn);
      for (int r = -1; r < reps; r++) { // one untimed pass first: both kernels
         HIP_CHECK(hipEventRecord(e0, ctx->stream));
         for (uint64_t a = 0; a < N; a += rows) pcr_products(ctx, s, true, a, std::min(a + rows, N), 0, std::min(a + rows, N), r < 0 ? 3 : what);
         HIP_CHECK(hipEventRecord(e1, ctx->stream));
         HIP_CHECK(hipEventSynchronize(e1));
         if (r >= 0) ms[r] = elapsed_ms(e0, e1);
      }
      if (flops) { // the 32 x 32 wave blocks on or below the diagonal, two Grams, each 2 x 32 x 32 flops per SNP slot
         const double nb = (double)((N + 31) / 32), blocks = nb * (nb + 1.0) / 2.0;
         *flops = blocks * 2.0 * 2.0 * 32.0 * 32.0 * (double)round_up(P, PCR_CHUNK);
      }
   });
}
