// pcrelate_ibd.hip -- PC-Relate IBD sharing: k2, k0 and the shared-SNP count of every pair, fpca_pcrelate_ibd_block / fpca_pcrelate_ibd_tri /
// fpca_pcrelate_classify (include/fpca.h "PC-Relate IBD sharing"), fpca_bench_pcrelate_ibd.
//
// beta, mu and the usable cells are pcrelate.hip's (pcrelate.hpp shares the host side).  Per usable (sample, SNP) cell, with mu its
// individual-specific allele frequency and x its dosage: v = mu (1 - mu), q = gD - v (gD = mu, 0, 1 - mu for x = 0, 1, 2), u = mu^2,
// t = (1 - mu)^2, s = [x = 0] - [x = 2], m = 1; all 0 at a cell that is not usable.  Seven products per pair:
//      Q = q q'    E = v v'    H1 = u t'    H2 = t u'    zz = s^2 (s^2)'    ss = s s'    n = m m'
// and k2 = Q / E - f_i f_j, k0 = I0 / (H1 + H2) with I0 = (zz - ss) / 2 the opposite homozygotes among the SNPs usable in both.
//   k_pcr_ibd_operands  k_pcr_operands' grid, staging and dot product; each cell is computed once and written to THREE panel arrays of
//                       16-byte pairs -- (q, v), (u, t), (s, m) -- in k_pcr_operands' layout: pair [(step * rows + p) * 16 + (snp ^ (p & 15))].
//   k_pcr_ibd           one template (ibd_tile_pair), k_pcr_gram's geometry (a 2 x 2 wave workgroup per pair of 64-sample tiles, 16-SNP steps
//                       through a 64 KB double buffer filled by linear 16-byte loads issued under the previous step's MFMAs, one
//                       conflict-free ds_read_b128 per sample and 4-SNP group, a triangle mode), three instances, each over its own panel
//                       array and staging, each with two accumulator sets (64 registers) so that two waves per SIMD stay resident; ONE
//                       launch runs all three, grid.y choosing the instance of a workgroup:
//                          IBD_QE   (q, v): Q += q q', E += v v'
//                          IBD_H    (u, t): H1 += u t', H2 += t u' -- the halves of H apart: (i, j) and (j, i) see the same two sums
//                          IBD_INT  (s, m): I2 += s^2 (s^2)' - s s' (s^2 formed in a register; small integers, exact in any order), n += m m'
//                       No atomics, no split along the SNPs: the accumulators live in the slab scratch between panels.
//   k_pcr_ibd_finish    the two divides (E == 0 and H == 0 tested: NaN), H1 + H2 added once, the f_i f_j correction as one rounded multiply
//                       and one rounded subtract (never fused), n converted to uint32; the rectangle or the packed triangle rows.
// Slabs of rows by a rule of this file: the six sums of a slab within 256 MiB; the three panels together within 1 GiB.
#include <algorithm>
#include <cmath>
#include <limits>

#include "ctx.hpp"
#include "launch_check.hpp"
#include "pcrelate.hpp"
#include "../../include/fpca_debug.h"

using namespace fpca;

namespace {

constexpr int IBD_QE = 0, IBD_H = 1, IBD_INT = 2;
constexpr int IBD_PANELS = 3; // (q, v), (u, t), (s, m)
constexpr int IBD_SUMS = 6;   // Q, E, H1, H2, I2, n

// k_pcr_operands' arguments and grid; panel row p holds sample s0 + p for p < n0 and sample s1 + (p - n0) after that
__global__ __launch_bounds__(256) void k_pcr_ibd_operands(const uint8_t *__restrict__ smp, size_t pitch, uint64_t N, const double *__restrict__ V,
                                                           const double *__restrict__ beta, const double *__restrict__ mean,
                                                           const double *__restrict__ sd, uint64_t P_g, int d, double lo, double hi, uint64_t snp0,
                                                           uint64_t s0, uint64_t n0, uint64_t s1, uint64_t rows, d2 *__restrict__ pqv,
                                                           d2 *__restrict__ put, d2 *__restrict__ psm)
{
#pragma clang fp contract(off)
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
         const double mu = 0.5 * acc;
         const bool usable = lv[sn] && code != 1u && mu > lo && mu < hi;
         d2 qv = d2{0.0, 0.0}, ut = d2{0.0, 0.0}, sm = d2{0.0, 0.0};
         if (usable) { // code 0: x = 2, code 2: x = 1, code 3: x = 0
            const double om = 1.0 - mu, v = mu * om, gd = code == 3u ? mu : code == 0u ? om : 0.0;
            qv.x = gd - v;
            qv.y = v;
            ut.x = mu * mu;
            ut.y = om * om;
            sm.x = code == 3u ? 1.0 : code == 0u ? -1.0 : 0.0;
            sm.y = 1.0;
         }
         const size_t at = (size_t)((((uint64_t)blockIdx.x * 4 + st) * rows + p) * PCR_STEP + t);
         pqv[at] = qv;
         put[at] = ut;
         psm[at] = sm;
      }
   }
}

// One workgroup's pair of tiles for one product set.  k_pcr_gram's arguments: workgroup w -> (tI, tJ) = (w / ntj, w % ntj); tile tI holds
// panel rows pa0 + 64 tI ..., tile tJ panel rows pb0 + 64 tJ ...; every tile lies within the panel's `rows` rows.  A0 and A1
// [(i - i0) * ld + (j - j0)] are the set's two sums, read back unless this is the first panel.  TRI: blocks wholly above the diagonal
// are skipped.  tile: [buffer][I, J][sample][slot], 64 KB.
template <bool TRI, int KIND>
__device__ __forceinline__ void ibd_tile_pair(d2 (*__restrict__ tile)[2][PCR_TILE * PCR_STEP], const d2 *__restrict__ panel, uint64_t rows, uint32_t nsteps,
                                              uint64_t pa0, uint64_t pb0, uint64_t i0, uint64_t iend, uint64_t j0, uint64_t jend, uint32_t ntj, int first,
                                              double *__restrict__ A0, double *__restrict__ A1, size_t ld)
{
   const uint64_t tI = blockIdx.x / ntj, tJ = blockIdx.x % ntj;
   if (TRI && j0 + tJ * PCR_TILE > i0 + tI * PCR_TILE + (PCR_TILE - 1)) return; // (uniform over the workgroup, before any barrier)
   const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, m = lane & 15, k = lane >> 4, wr = wave >> 1, wc = wave & 1;
   const uint64_t ia = i0 + tI * PCR_TILE + (uint64_t)wr * 32, ja = j0 + tJ * PCR_TILE + (uint64_t)wc * 32;
   const bool active = ia < iend && ja < jend && !(TRI && ja > ia + 31); // a wave without work still stages the tiles and meets the barriers
   const uint64_t pI = pa0 + tI * PCR_TILE, pJ = pb0 + tJ * PCR_TILE;
   const d2 *srcI = panel + pI * PCR_STEP + tid, *srcJ = panel + pJ * PCR_STEP + tid;
   const size_t stride = (size_t)rows * PCR_STEP;
   d4 c0[2][2], c1[2][2];
#pragma unroll
   for (int a = 0; a < 2; a++)
#pragma unroll
      for (int b = 0; b < 2; b++) {
         c0[a][b] = d4{0.0, 0.0, 0.0, 0.0};
         c1[a][b] = d4{0.0, 0.0, 0.0, 0.0};
         const uint64_t j = ja + 16 * b + m;
         if (first || !active || j >= jend) continue;
#pragma unroll
         for (int r = 0; r < 4; r++) {
            const uint64_t i = ia + 16 * a + k + 4 * r;
            if (i < iend) {
               c0[a][b][r] = A0[(size_t)(i - i0) * ld + (j - j0)];
               c1[a][b][r] = A1[(size_t)(i - i0) * ld + (j - j0)];
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
            d2 av[2], bv[2];
            av[0] = tA[snp ^ swA];
            av[1] = tA[16 * PCR_STEP + (snp ^ swA)];
            bv[0] = tB[snp ^ swB];
            bv[1] = tB[16 * PCR_STEP + (snp ^ swB)];
            if (KIND == IBD_QE) {
#pragma unroll
               for (int e = 0; e < 4; e++) {
                  c0[e >> 1][e & 1] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[e >> 1].x, bv[e & 1].x, c0[e >> 1][e & 1], 0, 0, 0);
                  c1[e >> 1][e & 1] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[e >> 1].y, bv[e & 1].y, c1[e >> 1][e & 1], 0, 0, 0);
               }
            } else if (KIND == IBD_H) {
#pragma unroll
               for (int e = 0; e < 4; e++) {
                  c0[e >> 1][e & 1] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[e >> 1].x, bv[e & 1].y, c0[e >> 1][e & 1], 0, 0, 0);
                  c1[e >> 1][e & 1] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[e >> 1].y, bv[e & 1].x, c1[e >> 1][e & 1], 0, 0, 0);
               }
            } else {
               // s in {-1, 0, 1}: s^2 and -s are exact; both products into one accumulator, the four blocks between them
               const double za[2] = {av[0].x * av[0].x, av[1].x * av[1].x}, zb[2] = {bv[0].x * bv[0].x, bv[1].x * bv[1].x};
               const double na[2] = {-av[0].x, -av[1].x};
#pragma unroll
               for (int e = 0; e < 4; e++) {
                  c0[e >> 1][e & 1] = __builtin_amdgcn_mfma_f64_16x16x4f64(za[e >> 1], zb[e & 1], c0[e >> 1][e & 1], 0, 0, 0);
                  c1[e >> 1][e & 1] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[e >> 1].y, bv[e & 1].y, c1[e >> 1][e & 1], 0, 0, 0);
               }
#pragma unroll
               for (int e = 0; e < 4; e++)
                  c0[e >> 1][e & 1] = __builtin_amdgcn_mfma_f64_16x16x4f64(na[e >> 1], bv[e & 1].x, c0[e >> 1][e & 1], 0, 0, 0);
            }
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
               A0[(size_t)(i - i0) * ld + (j - j0)] = c0[a][b][r];
               A1[(size_t)(i - i0) * ld + (j - j0)] = c1[a][b][r];
            }
         }
      }
}

struct IbdPanels {
   const d2 *qv, *ut, *sm;
};

struct IbdAcc {
   double *Q, *E, *H1, *H2, *I2, *n;
};

// grid: x = the tile pairs, y = the product set (IBD_QE, IBD_H, IBD_INT): the three instances of ibd_tile_pair in ONE launch, so that the
// workgroups of a slab -- few, where its six sums must fit 256 MiB -- fill the device three times as far before the last round
template <bool TRI>
__global__ __launch_bounds__(256, 2) void k_pcr_ibd(IbdPanels p, uint64_t rows, uint32_t nsteps, uint64_t pa0, uint64_t pb0, uint64_t i0, uint64_t iend,
                                                    uint64_t j0, uint64_t jend, uint32_t ntj, int first, IbdAcc s, size_t ld)
{
   __shared__ d2 tile[2][2][PCR_TILE * PCR_STEP];
   if (blockIdx.y == IBD_QE) // (uniform over the workgroup)
      ibd_tile_pair<TRI, IBD_QE>(tile, p.qv, rows, nsteps, pa0, pb0, i0, iend, j0, jend, ntj, first, s.Q, s.E, ld);
   else if (blockIdx.y == IBD_H)
      ibd_tile_pair<TRI, IBD_H>(tile, p.ut, rows, nsteps, pa0, pb0, i0, iend, j0, jend, ntj, first, s.H1, s.H2, ld);
   else
      ibd_tile_pair<TRI, IBD_INT>(tile, p.sm, rows, nsteps, pa0, pb0, i0, iend, j0, jend, ntj, first, s.I2, s.n, ld);
}

struct IbdSums {
   const double *Q, *E, *H1, *H2, *I2, *n;
};

// one thread per cell (a, b) of the slab: sample i = i0 + a (row), sample j = j0 + b (column).  RECT: out[a * ld + b]; TRI: the columns
// start at sample 0, out[i (i + 1) / 2 + b - i0 (i0 + 1) / 2] for b <= i.  f and each output may be null.
template <int MODE>
__global__ __launch_bounds__(256) void k_pcr_ibd_finish(IbdSums s, size_t ld, uint64_t i0, uint64_t ni, uint64_t j0, uint64_t nj,
                                                         const double *__restrict__ f, double *__restrict__ k2, double *__restrict__ k0,
                                                         uint32_t *__restrict__ nsnp)
{
#pragma clang fp contract(off) // the product f_i f_j is rounded before it is subtracted
   const uint64_t b = (uint64_t)blockIdx.x * 256 + threadIdx.x, a = blockIdx.y;
   if (b >= nj || a >= ni) return;
   const uint64_t i = i0 + a, j = j0 + b;
   if (MODE == PCR_TRI && b > i) return;
   const size_t at = (size_t)a * ld + b;
   const size_t o = MODE == PCR_RECT ? at : (size_t)(i * (i + 1) / 2 - i0 * (i0 + 1) / 2 + b);
   if (k2) {
      const double e = s.E[at], ff = f ? f[i] * f[j] : 0.0, qe = s.Q[at] / e;
      k2[o] = e == 0.0 ? __builtin_nan("") : qe - ff;
   }
   if (k0) {
      const double h = s.H1[at] + s.H2[at];
      k0[o] = h == 0.0 ? __builtin_nan("") : (0.5 * s.I2[at]) / h; // (the halving of an even integer is exact)
   }
   if (nsnp) nsnp[o] = (uint32_t)s.n[at];
}

// ---- host ---------------------------------------------------------------------------------------------------------------

// device buffers of one call: PcrBufs' sample-major copy, V and beta; the three panels, the six sums and the outputs of a slab
struct IbdBufs {
   PcrBufs base;
   DevMem<d2> panel[IBD_PANELS];
   uint64_t panel_snps = 0, panel_rows = 0;
   DevMem<double> sum[IBD_SUMS], d_f, d_k2, d_k0;
   DevMem<uint32_t> d_n;
   size_t ld = 0;
};

// rows of a slab whose cells are `cols` wide: the six sums within PCR_SLAB_BYTES, the tile pairs within one launch; whole tiles, at least one
uint64_t ibd_slab_rows(uint64_t cols)
{
   if (const uint64_t forced = PCR_ENV("FPCA_PCR_SLAB_ROWS", PCR_TILE)) return forced;
   const uint64_t by_mem = PCR_SLAB_BYTES / (cols * IBD_SUMS * sizeof(double)) / PCR_TILE;
   const uint64_t by_launch = PCR_LAUNCH_PAIRS / ((cols + PCR_TILE - 1) / PCR_TILE);
   return std::min<uint64_t>(std::max<uint64_t>(std::min(by_mem, by_launch), 1), 512) * PCR_TILE; // (a row is one grid.y of the finish kernel)
}

uint64_t ibd_tri_rows(uint64_t N) { return std::min<uint64_t>(ibd_slab_rows(N), round_up(N, PCR_TILE)); }

// the three panels for slabs that need up to `rows` panel rows: as many whole chunks as PCR_PANEL_BYTES holds for the three, at least one
void ibd_alloc_panels(const fpca_ctx *c, IbdBufs &s, uint64_t rows, const char *fn)
{
   const uint64_t slots = round_up(c->P_g, PCR_CHUNK);
   uint64_t snps = PCR_ENV("FPCA_PCR_PANEL_SNPS", PCR_CHUNK);
   if (!snps) snps = PCR_PANEL_BYTES / (rows * sizeof(d2) * IBD_PANELS) / PCR_CHUNK * PCR_CHUNK;
   if (!snps)
      throw Error(FPCA_ENOMEM, std::string(fn) + ": three panels of " + std::to_string(PCR_CHUNK) + " SNPs x " + std::to_string(rows) + " samples need " +
                                   std::to_string(rows * sizeof(d2) * IBD_PANELS * PCR_CHUNK) + " bytes, the panels are capped at " +
                                   std::to_string(PCR_PANEL_BYTES) + "; call fpca_pcrelate_ibd_block on fewer samples at a time");
   s.panel_snps = std::min(snps, slots);
   s.panel_rows = rows;
   static const char *const what[IBD_PANELS] = {"operand panel (q, v)", "operand panel (u, t)", "operand panel (s, m)"};
   char detail[128];
   std::snprintf(detail, sizeof(detail), "one of three panels of %llu SNPs x %llu samples", (unsigned long long)s.panel_snps, (unsigned long long)rows);
   for (int a = 0; a < IBD_PANELS; a++) s.panel[a] = DevMem<d2>((size_t)s.panel_snps * rows, fn, what[a], 0, detail, c->device);
}

void ibd_alloc_slab(const fpca_ctx *c, IbdBufs &s, uint64_t rows, uint64_t cols, bool k2, bool k0, bool nsnp, const char *fn)
{
   s.ld = (size_t)cols;
   const size_t cells = (size_t)rows * cols;
   static const char *const what[IBD_SUMS] = {"slab scratch (Q)", "slab scratch (E)", "slab scratch (H, first half)", "slab scratch (H, second half)",
                                              "slab scratch (opposite homozygotes)", "slab scratch (shared SNPs)"};
   char detail[128];
   std::snprintf(detail, sizeof(detail), "one of six sums of a slab of %llu rows x %llu samples", (unsigned long long)rows, (unsigned long long)cols);
   for (int a = 0; a < IBD_SUMS; a++) s.sum[a] = DevMem<double>(cells, fn, what[a], 0, detail, c->device);
   if (k2) s.d_k2 = DevMem<double>(cells, fn, "slab scratch (k2)", 0, detail, c->device);
   if (k0) s.d_k0 = DevMem<double>(cells, fn, "slab scratch (k0)", 0, detail, c->device);
   if (nsnp) s.d_n = DevMem<uint32_t>(cells, fn, "slab scratch (nsnp)", 0, detail, c->device);
}

// the six sums of the cells [i0, iend) x [j0, jend) into the slab scratch: per panel, the operands, then the three Gram instances.  what:
// 3 all kernels, 1 the operand kernel alone, 2 the Gram instances alone (on whatever the panels hold: the bench hook)
void ibd_products(const fpca_ctx *c, const IbdBufs &s, bool tri, uint64_t i0, uint64_t iend, uint64_t j0, uint64_t jend, int what = 3)
{
   const uint64_t nti = (iend - i0 + PCR_TILE - 1) / PCR_TILE, ntj = (jend - j0 + PCR_TILE - 1) / PCR_TILE, wgs = nti * ntj;
   if (!wgs) return;
   if (wgs > 0x7FFFFFFFull || ntj > 0xFFFFFFFFull) throw Error(FPCA_EINVAL, "PC-Relate IBD: " + std::to_string(wgs) + " tile pairs exceed one launch");
   const PcrMap mp = pcr_map(i0, iend, j0, jend);
   if (mp.rows > s.panel_rows) throw Error(FPCA_EHIP, "PC-Relate IBD: a slab needs more panel rows than were allocated");
   const PcrBufs &b = s.base;
   const uint64_t slots = round_up(c->P_g, PCR_CHUNK);
   for (uint64_t snp0 = 0; snp0 < slots; snp0 += s.panel_snps) {
      const uint64_t cc = std::min(s.panel_snps, slots - snp0);
      if (what & 1) {
         hipLaunchKernelGGL(k_pcr_ibd_operands, dim3((unsigned)(cc / PCR_BLK_SNPS), (unsigned)((mp.rows + PCR_BLK_SNPS - 1) / PCR_BLK_SNPS)), dim3(256), 0,
                            c->stream, b.d_smp.p, b.pitch, c->N, b.d_V.p, b.d_beta.p, c->d_mean, c->d_sd, c->P_g, b.d, b.lo, b.hi, snp0, mp.s0, mp.n0,
                            mp.s1, mp.rows, s.panel[0].p, s.panel[1].p, s.panel[2].p);
         launch_check();
      }
      if (what & 2) {
         const IbdPanels pn{s.panel[0].p, s.panel[1].p, s.panel[2].p};
         const IbdAcc acc{s.sum[0].p, s.sum[1].p, s.sum[2].p, s.sum[3].p, s.sum[4].p, s.sum[5].p};
         const dim3 grid((unsigned)wgs, IBD_PANELS);
         if (tri)
            hipLaunchKernelGGL(k_pcr_ibd<true>, grid, dim3(256), 0, c->stream, pn, mp.rows, (uint32_t)(cc / PCR_STEP), mp.pa0, mp.pb0, i0, iend, j0, jend,
                               (uint32_t)ntj, (int)(snp0 == 0), acc, s.ld);
         else
            hipLaunchKernelGGL(k_pcr_ibd<false>, grid, dim3(256), 0, c->stream, pn, mp.rows, (uint32_t)(cc / PCR_STEP), mp.pa0, mp.pb0, i0, iend, j0, jend,
                               (uint32_t)ntj, (int)(snp0 == 0), acc, s.ld);
         launch_check();
      }
   }
}

void ibd_finish(int mode, const fpca_ctx *c, const IbdBufs &s, uint64_t i0, uint64_t ni, uint64_t j0, uint64_t nj)
{
   const dim3 grid((unsigned)((nj + 255) / 256), (unsigned)ni), block(256);
   const IbdSums sums{s.sum[0].p, s.sum[1].p, s.sum[2].p, s.sum[3].p, s.sum[4].p, s.sum[5].p};
   if (mode == PCR_RECT)
      hipLaunchKernelGGL(k_pcr_ibd_finish<PCR_RECT>, grid, block, 0, c->stream, sums, s.ld, i0, ni, j0, nj, s.d_f.p, s.d_k2.p, s.d_k0.p, s.d_n.p);
   else
      hipLaunchKernelGGL(k_pcr_ibd_finish<PCR_TRI>, grid, block, 0, c->stream, sums, s.ld, i0, ni, j0, nj, s.d_f.p, s.d_k2.p, s.d_k0.p, s.d_n.p);
   launch_check();
}

void ibd_download(const fpca_ctx *c, const IbdBufs &s, size_t at, size_t cells, double *k2, double *k0, uint32_t *nsnp)
{
   if (k2) HIP_CHECK(hipMemcpyAsync(k2 + at, s.d_k2.p, cells * sizeof(double), hipMemcpyDeviceToHost, c->stream));
   if (k0) HIP_CHECK(hipMemcpyAsync(k0 + at, s.d_k0.p, cells * sizeof(double), hipMemcpyDeviceToHost, c->stream));
   if (nsnp) HIP_CHECK(hipMemcpyAsync(nsnp + at, s.d_n.p, cells * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
}

// what fpca_pcrelate_ibd_block and fpca_pcrelate_ibd_tri share.  Everything up to pcr_make_operand is host work: every refusal comes first.
void ibd_run(fpca_ctx *ctx, const char *fn, int mode, const double *pcs, int npc, const double *beta, const uint8_t *train, double eps, const double *f,
             uint64_t i0, uint64_t ni, uint64_t j0, uint64_t nj, double *k2, double *k0, uint32_t *nsnp)
{
   pcr_refuse(ctx, fn);
   if (!k2 && !k0 && !nsnp) throw Error(FPCA_EINVAL, std::string("bad argument to ") + fn + " (k2, k0 and nsnp are all NULL)");
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
   if (f)
      for (uint64_t i = 0; i < N; i++)
         if (!std::isfinite(f[i])) throw Error(FPCA_EINVAL, std::string(fn) + ": f[" + std::to_string(i) + "] is not finite");
   std::vector<double> lc;
   if (beta) {
      for (size_t e = 0; e < (size_t)ctx->P_g * d; e++)
         if (!std::isfinite(beta[e]))
            throw Error(FPCA_EINVAL, std::string(fn) + ": beta[" + std::to_string(e / d) + "][" + std::to_string(e % d) + "] is not finite");
   } else {
      pcr_factor(ctx, fn, V, d, train, lc);
   }
   HIP_CHECK(hipSetDevice(ctx->device));
   IbdBufs s;
   s.base.lo = eps;
   s.base.hi = 1.0 - eps;
   pcr_make_operand(ctx, s.base, fn, V, d, beta);
   if (!beta) pcr_beta_dev(ctx, fn, V, d, train, lc, s.base.d_beta.p);
   if (f && k2) {
      s.d_f = DevMem<double>((size_t)N, fn, "the inbreeding coefficients");
      HIP_CHECK(hipMemcpyAsync(s.d_f.p, f, (size_t)N * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
   }
   if (mode == PCR_RECT) {
      const uint64_t rows = std::min<uint64_t>(ibd_slab_rows(nj), round_up(ni, PCR_TILE));
      ibd_alloc_panels(ctx, s, rows + round_up(nj, PCR_TILE), fn);
      ibd_alloc_slab(ctx, s, rows, nj, k2 != nullptr, k0 != nullptr, nsnp != nullptr, fn);
      for (uint64_t a = i0; a < i0 + ni; a += rows) {
         const uint64_t b = std::min(a + rows, i0 + ni);
         ibd_products(ctx, s, false, a, b, j0, j0 + nj);
         ibd_finish(PCR_RECT, ctx, s, a, b - a, j0, nj);
         ibd_download(ctx, s, (size_t)(a - i0) * nj, (size_t)(b - a) * nj, k2, k0, nsnp);
      }
   } else {
      const uint64_t rows = ibd_tri_rows(N);
      ibd_alloc_panels(ctx, s, round_up(N, PCR_TILE), fn);
      ibd_alloc_slab(ctx, s, rows, N, k2 != nullptr, k0 != nullptr, nsnp != nullptr, fn);
      for (uint64_t a = 0; a < N; a += rows) {
         const uint64_t b = std::min(a + rows, N);
         const size_t at = (size_t)(a * (a + 1) / 2), cells = (size_t)(b * (b + 1) / 2) - at; // the packed rows a .. b - 1
         ibd_products(ctx, s, true, a, b, 0, b);
         ibd_finish(PCR_TRI, ctx, s, a, b - a, 0, b);
         // the slab goes to the host as it finishes; the next one's kernels queue behind the copy
         ibd_download(ctx, s, at, cells, k2, k0, nsnp);
      }
   }
   HIP_CHECK(hipStreamSynchronize(ctx->stream));
}

} // namespace

extern "C" int fpca_pcrelate_ibd_block(fpca_ctx *ctx, const double *pcs, int npc, const double *beta, const uint8_t *train, double eps, const double *f,
                                       uint64_t i0, uint64_t ni, uint64_t j0, uint64_t nj, double *k2, double *k0, uint32_t *nsnp)
{
   return guarded([&] { ibd_run(ctx, "fpca_pcrelate_ibd_block", PCR_RECT, pcs, npc, beta, train, eps, f, i0, ni, j0, nj, k2, k0, nsnp); });
}

extern "C" int fpca_pcrelate_ibd_tri(fpca_ctx *ctx, const double *pcs, int npc, const double *beta, const uint8_t *train, double eps, const double *f,
                                     double *k2, double *k0, uint32_t *nsnp)
{
   return guarded([&] { ibd_run(ctx, "fpca_pcrelate_ibd_tri", PCR_TRI, pcs, npc, beta, train, eps, f, 0, 0, 0, 0, k2, k0, nsnp); });
}

extern "C" int fpca_pcrelate_classify(uint64_t n_pairs, const double *kin, const double *k0, const double *k2, const uint32_t *nsnp, double k0_switch,
                                      double po_k0, double *k0_out, double *k1_out, uint8_t *type)
{
   return guarded([&] {
      if (n_pairs && (!kin || !k0 || !k2 || !nsnp || !k0_out || !k1_out || !type))
         throw Error(FPCA_EINVAL, "bad argument to fpca_pcrelate_classify (a NULL array)");
      if (!std::isfinite(k0_switch)) throw Error(FPCA_EINVAL, "fpca_pcrelate_classify: k0_switch is not a finite number");
      if (!std::isfinite(po_k0)) throw Error(FPCA_EINVAL, "fpca_pcrelate_classify: po_k0 is not a finite number");
      for (uint64_t p = 0; p < n_pairs; p++) {
         const double v = kin[p];
         // 4 kin is exact, so a fused 1 - 4 kin is the rounded difference; the other steps are sums alone
         const double z0 = v > k0_switch ? k0[p] : (1.0 - 4.0 * v) + k2[p];
         k0_out[p] = z0;
         k1_out[p] = (1.0 - z0) - k2[p];
         uint8_t t = 0;
         if (std::isnan(v) || std::isnan(z0) || nsnp[p] == 0)
            t = 255;
         else if (v > 0.354)
            t = 5;
         else if (v > 0.177)
            t = z0 < po_k0 ? 1 : 2;
         else if (v > 0.0884)
            t = 3;
         else if (v > 0.0442)
            t = 4;
         type[p] = t;
      }
   });
}

extern "C" int fpca_bench_pcrelate_ibd(fpca_ctx *ctx, int npc, int reps, double *ms, double *flops)
{
   return guarded([&] {
      const char *fn = "fpca_bench_pcrelate_ibd";
      pcr_refuse(ctx, fn);
      if (!ms || reps < 1 || npc < 0 || npc > PCR_MAXD - 1) throw Error(FPCA_EINVAL, "bad argument to fpca_bench_pcrelate_ibd");
      HIP_CHECK(hipSetDevice(ctx->device));
      const uint64_t N = ctx->N, P = ctx->P_g;
      const int d = npc + 1;
      // fpca_bench_pcrelate's model: every called entry of a live SNP usable, mu = 0.5 + 0.01 sum_k V_ik, |V_ik| <= 1 / npc
      std::vector<double> V((size_t)N * d), beta((size_t)P * d);
      for (uint64_t i = 0; i < N; i++) {
         V[(size_t)i * d] = 1.0;
         for (int k = 1; k < d; k++) V[(size_t)i * d + k] = (double)((int)((i * 7 + k * 13) % 21) - 10) / (10.0 * npc);
      }
      for (uint64_t j = 0; j < P; j++) {
         beta[(size_t)j * d] = 1.0;
         for (int k = 1; k < d; k++) beta[(size_t)j * d + k] = 0.02;
      }
      IbdBufs s;
      s.base.lo = 0.01;
      s.base.hi = 0.99;
      pcr_make_operand(ctx, s.base, fn, V, d, beta.data());
      const uint64_t rows = ibd_tri_rows(N);
      ibd_alloc_panels(ctx, s, round_up(N, PCR_TILE), fn);
      ibd_alloc_slab(ctx, s, rows, N, false, false, false, fn);
      // the three Gram instances alone over the whole triangle, slab by slab and panel by panel as fpca_pcrelate_ibd_tri launches them, on
      // the panels the untimed pass left (test build, FPCA_PCR_BENCH_OPERANDS=1: the operand kernel alone instead)
      const char *v = FPCA_TEST_ENV("FPCA_PCR_BENCH_OPERANDS");
      const int what = (v && *v && *v != '0') ? 1 : 2;
      DevEvent e0(fn), e1(fn);
      for (int r = -1; r < reps; r++) { // one untimed pass first: all kernels
         HIP_CHECK(hipEventRecord(e0, ctx->stream));
         for (uint64_t a = 0; a < N; a += rows) ibd_products(ctx, s, true, a, std::min(a + rows, N), 0, std::min(a + rows, N), r < 0 ? 3 : what);
         HIP_CHECK(hipEventRecord(e1, ctx->stream));
         HIP_CHECK(hipEventSynchronize(e1));
         if (r >= 0) ms[r] = elapsed_ms(e0, e1);
      }
      if (flops) { // the 32 x 32 wave blocks on or below the diagonal, seven products, each 2 x 32 x 32 flops per SNP slot
         const double nb = (double)((N + 31) / 32), blocks = nb * (nb + 1.0) / 2.0;
         *flops = blocks * 7.0 * 2.0 * 32.0 * 32.0 * (double)round_up(P, PCR_CHUNK);
      }
   });
}
