// ld_band.hip -- LD pruning: fpca_ld_band / fpca_ld_prune (include/fpca.h "LD pruning"), fpca_debug_ld_prune_rule / fpca_bench_ld.
//
// Windowed pairwise r2 is a BANDED GRAM of the integer genotype matrix with itself: both operands are the SNP-major 2-bit records the
// context holds (K = samples, contiguous), decoded with the v_perm table trick of kernels_i8.hip (i8_decode) into int8 planes
//      x = dosage (0 where missing)   table 0x00010002        q = x^2   table 0x00010004        e = 1 - m (missing)   table 0x00000100
// and multiplied on v_mfma_i32_32x32x32_i8 with exact int32 sums.  Nothing is sliced, nothing is rounded before the final quotient.
//   k_ld_totals   per record: sum x, sum x^2, sum e over the `pitch` bytes (pad samples are code "01": they count in sum e).
//   k_ld_band     one workgroup (4 waves, 2 x 2) per pair of 64-SNP tiles (I, J), J >= I, whose index ranges come within `span` of each
//                 other; a wave owns one 32 x 32 block of pairs and SIX accumulator planes for it (x.x, x.e, e.x, q.e, e.q, e.e: 96
//                 accumulator registers).  A lane reads 64 contiguous bytes of its record per chunk (lanes l and l + 32 share a 128-byte
//                 line: every line is requested once), straight into registers on both sides -- no LDS: six products per loaded pair
//                 put the kernel at 1/6 of a plain GEMM's operand traffic per MFMA, and the next chunk's loads are issued before this
//                 chunk's 96 MFMAs.  A wave whose two 32-record blocks hold no missing call (sum e == pad samples, from k_ld_totals)
//                 multiplies x.x only: e is then 1 exactly at the pad samples of both sides, where x = q = 0, so the four mixed
//                 products are 0 and e.e is the pad count -- the same integers, hence the same bits.  The kernel knows nothing about
//                 windows, steps, chromosomes or `keep`: it computes every pair with 1 <= j - i <= span.  No split-K: at the sizes the
//                 feature is for there are thousands of tile pairs; a small P under-fills the device, which is accepted.
//                 Epilogue BAND: r2[i][j - i - 1] as fp64.  Epilogue BITS: bit j - i - 1 of row i of a bitmap that the caller zeroed,
//                 set with atomicOr (a vector-memory atomic) when r2 > thr -- a tile pair covers only part of a row's words.
// The pruning rule runs on the host (ld_prune_rule): it is a sequential greedy pass, and the bitmap is 12.5 MB at 100,000 x 999.
#include <algorithm>
#include <chrono>
#include <cmath>

#include "ctx.hpp"
#include "launch_check.hpp"
#include "ld_planes.hpp"

using namespace fpca;

namespace {

constexpr int LD_TILE = 64;                        // records per workgroup tile side (2 waves x 32)
constexpr uint64_t LD_MAX_N = 1ull << 25;          // 4 N^2 < 2^53: every integer of the statistic is exact in a double
constexpr uint64_t LD_BAND_LIMIT = 1ull << 30;     // bytes of an fpca_ld_band buffer
constexpr uint64_t LD_BITS_SLAB = 256ull << 20;    // bytes of one slab of the fpca_ld_prune bitmap

// one wave per record: counts of code 00 (x = 2), 10 (x = 1) and 01 (missing / pad) over the whole pitch
__global__ __launch_bounds__(256) void k_ld_totals(const uint8_t *__restrict__ packed, size_t pitch, uint64_t nrec, uint32_t *__restrict__ tot)
{
   const uint64_t rec = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
   if (rec >= nrec) return; // (wave-uniform; no barrier below)
   const int lane = threadIdx.x & 63;
   const uint4 *row = reinterpret_cast<const uint4 *>(packed + rec * pitch);
   const uint32_t nv = (uint32_t)(pitch / 16);
   uint32_t c2 = 0, c1 = 0, ce = 0;
   for (uint32_t v = lane; v < nv; v += 64) {
      const uint4 p = row[v];
      const uint32_t w[4] = {p.x, p.y, p.z, p.w};
#pragma unroll
      for (int d = 0; d < 4; d++) {
         const uint32_t lo = w[d] & 0x55555555u, hi = (w[d] >> 1) & 0x55555555u;
         c2 += __popc(~lo & ~hi & 0x55555555u);
         c1 += __popc(hi & ~lo);
         ce += __popc(lo & ~hi);
      }
   }
#pragma unroll
   for (int o = 32; o > 0; o >>= 1) {
      c2 += __shfl_down(c2, o, 64);
      c1 += __shfl_down(c1, o, 64);
      ce += __shfl_down(ce, o, 64);
   }
   if (lane == 0) reinterpret_cast<uint4 *>(tot)[rec] = make_uint4(2 * c2 + c1, 4 * c2 + c1, ce, 0u);
}

// tiles are counted from i0: tile t holds records [i0 + 64 t, i0 + 64 t + 64); workgroup w -> (tI, tJ) = (w / nj, w / nj + w % nj)
template <bool BAND>
__global__ __launch_bounds__(256, 2) void k_ld_band(const uint8_t *__restrict__ packed, size_t pitch, const uint32_t *__restrict__ tot, uint32_t npad,
                                                    uint64_t i0, uint64_t ni, uint64_t jend, uint32_t span, uint32_t nj, double *__restrict__ r2,
                                                    uint32_t *__restrict__ bits, uint32_t words, double thr, int force_general)
{
   const uint64_t tI = blockIdx.x / nj, tJ = tI + blockIdx.x % nj;
   const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, li = lane & 31, kh = lane >> 5;
   // this wave's 32 x 32 block of pairs: records ia .. ia + 31 (MFMA operand A, output rows) x ja .. ja + 31 (operand B, output columns)
   const uint64_t ia = i0 + tI * LD_TILE + (uint64_t)(wave >> 1) * 32, ja = i0 + tJ * LD_TILE + (uint64_t)(wave & 1) * 32, iend = i0 + ni;
   // nothing to do (wave-uniform; the kernel has no barrier): the block lies past the data, on or below the diagonal, or beyond the band
   if (ia >= iend || ja >= jend || ja + 31 <= ia || (ja > ia + 31 && ja - (ia + 31) > span)) return;
   // records past the last one are read as the last one (their pairs are dropped in the epilogue): no load leaves [0, jend)
   const uint64_t ra = ia + li < jend ? ia + li : jend - 1, rb = ja + li < jend ? ja + li : jend - 1;
   const uint4 ta = reinterpret_cast<const uint4 *>(tot)[ra], tb = reinterpret_cast<const uint4 *>(tot)[rb]; // (sum x, sum x^2, sum e, -)
   const bool general = force_general || __builtin_amdgcn_ballot_w64(ta.z != npad || tb.z != npad) != 0ull;
   const uint4 *pa = reinterpret_cast<const uint4 *>(packed + ra * pitch) + kh * 4;
   const uint4 *pb = reinterpret_cast<const uint4 *>(packed + rb * pitch) + kh * 4;
   const uint32_t nchunks = (uint32_t)(pitch / 128);
   v16i acc[6];
#pragma unroll
   for (int m = 0; m < 6; m++)
#pragma unroll
      for (int r = 0; r < 16; r++) acc[m][r] = 0;
   if (general) {
      ld_products<true, true>(pa, pb, nchunks, acc);
   } else {
      ld_products<false, true>(pa, pb, nchunks, acc);
#pragma unroll
      for (int r = 0; r < 16; r++) acc[5][r] = (int)npad; // e.e: the pad samples of both records; x.e = e.x = q.e = e.q = 0 stay
   }
   // Epilogue.  The planes hold sums over ALL 4 pitch sample slots, pad samples included, and e = 1 - m, so with the padded totals
   // Se = sum e (missing calls + pad samples), Sx = sum x, Sq = sum x^2 of a record and N_tot = 4 pitch:
   //    n   = sum m_i m_j = sum (1 - e_i)(1 - e_j) = N_tot - Se_i - Se_j + e_i.e_j     (pad samples: 1 - 1 - 1 + 1 = 0, as they must)
   //    sx  = sum x_i m_j = Sx_i - x_i.e_j            sy  = sum m_i x_j = Sx_j - e_i.x_j
   //    sxx = sum q_i m_j = Sq_i - q_i.e_j            syy = sum m_i q_j = Sq_j - e_i.q_j        sxy = x_i.x_j  (x = 0 where missing)
   // All of it exact in int64; the quotient is two multiplies and one divide in fp64, no add beside a multiply (nothing can fuse).
   const int64_t ntot = (int64_t)(4 * pitch);
   const uint64_t j = ja + li;
#pragma unroll
   for (int r = 0; r < 16; r++) {
      const int row = (r & 3) + 8 * (r >> 2) + 4 * kh; // v_mfma_i32_32x32x32_i8: register r of lane (li, kh) is D[row][li]
      const uint64_t i = ia + row;
      if (i >= iend || j >= jend || j <= i || j - i > span) continue;
      const uint4 ti = reinterpret_cast<const uint4 *>(tot)[i];
      const int64_t n = ntot - (int64_t)ti.z - (int64_t)tb.z + acc[5][r];
      const int64_t sx = (int64_t)ti.x - acc[1][r], sy = (int64_t)tb.x - acc[2][r], sxy = acc[0][r];
      const int64_t sxx = (int64_t)ti.y - acc[3][r], syy = (int64_t)tb.y - acc[4][r];
      const int64_t cv = n * sxy - sx * sy, vx = n * sxx - sx * sx, vy = n * syy - sy * sy;
      const double v = ((double)cv * (double)cv) / ((double)vx * (double)vy);
      const uint64_t d = j - i - 1;
      if (BAND) {
         r2[(size_t)(i - i0) * span + d] = v;
      } else if (v > thr) {
         atomicOr(&bits[(size_t)(i - i0) * words + (d >> 5)], 1u << (d & 31));
      }
   }
}

uint32_t ld_nj(uint32_t span) { return (uint32_t)(((uint64_t)span + LD_TILE - 1) / LD_TILE + 1); } // J tiles a tile I can reach

// what both entry points refuse (before any device work)
void ld_refuse(const fpca_ctx *c, const char *fn, bool needs_maf)
{
   if (!c) throw Error(FPCA_EINVAL, std::string("bad argument to ") + fn + " (NULL context)");
   if (c->dense)
      throw Error(FPCA_EINVAL, std::string(fn) + ": this context holds a dense matrix; r2 is computed from the packed genotypes (fpca_create, "
                                                 "fpca_create_from_bed, synthetic)");
   if (c->masked())
      throw Error(FPCA_EINVAL, std::string(fn) + ": a sample mask is set (fpca_set_sample_mask); r2 here is over all N samples -- clear the mask first");
   if (c->multi() || (c->rank_known && c->nranks > 1))
      throw Error(FPCA_EINVAL, std::string(fn) + ": this context is one shard of several (a communicator, an all-reduce hook or fpca_set_rank with "
                                                 "more than one rank); windows would end at the shard's edge -- prune on a single context");
   if (needs_maf && c->meansd_preloaded)
      throw Error(FPCA_EINVAL, std::string(fn) + ": this context carries a preloaded mean/sd (fpca_set_meansd); the rule compares K1's allele frequencies");
   if (c->N > LD_MAX_N)
      throw Error(FPCA_EINVAL, std::string(fn) + ": " + std::to_string(c->N) + " samples; above 2^25 = 33,554,432 the integers of r2 no longer fit 53 bits");
}

bool ld_force_general()
{
   const char *v = FPCA_TEST_ENV("FPCA_LD_FORCE_GENERAL");
   return v && *v && *v != '0';
}

// device buffers of one call
struct LdBufs {
   DevMem<uint32_t> d_tot, d_bits;
};

// totals of records [r0, r0 + nrec), at their own record numbers (the kernel indexes them absolutely)
void ld_make_totals(fpca_ctx *c, LdBufs &s, const char *fn, uint64_t r0, uint64_t nrec)
{
   s.d_tot = DevMem<uint32_t>(c->P_g * 4, fn, "the per-SNP totals");
   kern::ld_totals(c->d_packed + r0 * c->pitch, c->pitch, nrec, s.d_tot.p + r0 * 4, c->stream);
}

void ld_alloc_bits(fpca_ctx *c, LdBufs &s, const char *fn, uint64_t rows, uint32_t words)
{
   char detail[96];
   std::snprintf(detail, sizeof(detail), "%llu SNPs x %u words", (unsigned long long)rows, words);
   s.d_bits = DevMem<uint32_t>((size_t)rows * words, fn, "band bitmap", 0, detail, c->device);
}

} // namespace

namespace fpca {
namespace kern {

void ld_totals(const uint8_t *packed, size_t pitch, uint64_t nrec, uint32_t *tot, hipStream_t stream)
{
   if (!nrec) return;
   hipLaunchKernelGGL(k_ld_totals, dim3((unsigned)((nrec + 3) / 4)), dim3(256), 0, stream, packed, pitch, nrec, tot);
   launch_check();
}

void ld_band(const uint8_t *packed, size_t pitch, const uint32_t *tot, uint32_t npad, uint64_t i0, uint64_t ni, uint64_t jend, uint32_t span,
             double *r2, uint32_t *bits, uint32_t words, double thr, bool force_general, hipStream_t stream)
{
   if (!ni || !span || i0 + 1 >= jend) return;
   const uint64_t ti = (ni + LD_TILE - 1) / LD_TILE, nj = ld_nj(span), wgs = ti * nj;
   if (wgs > 0x7FFFFFFFull) throw Error(FPCA_EINVAL, "LD band: " + std::to_string(wgs) + " tile pairs exceed one launch; use a smaller range or span");
   if (r2)
      hipLaunchKernelGGL(k_ld_band<true>, dim3((unsigned)wgs), dim3(256), 0, stream, packed, pitch, tot, npad, i0, ni, jend, span, (uint32_t)nj, r2, bits,
                         words, thr, (int)force_general);
   else
      hipLaunchKernelGGL(k_ld_band<false>, dim3((unsigned)wgs), dim3(256), 0, stream, packed, pitch, tot, npad, i0, ni, jend, span, (uint32_t)nj, r2, bits,
                         words, thr, (int)force_general);
   launch_check();
}

} // namespace kern

void ld_check_window(const char *fn, uint32_t window, uint32_t step)
{
   if (window < 2) throw Error(FPCA_EINVAL, std::string(fn) + ": window = " + std::to_string(window) + "; a window holds at least 2 SNPs");
   if (step < 1) throw Error(FPCA_EINVAL, std::string(fn) + ": step = 0; windows advance by at least 1 SNP");
   if (step > window)
      throw Error(FPCA_EINVAL, std::string(fn) + ": step = " + std::to_string(step) + " is larger than window = " + std::to_string(window) +
                                   "; SNPs between two windows would never be compared");
}

uint64_t ld_prune_rule(const uint32_t *bits, uint32_t words, uint64_t P, uint32_t window, uint32_t step, const uint64_t *totals, const double *maf,
                       const uint32_t *chrom, uint8_t *keep)
{
   // non-candidates: cleared on entry, or monomorphic over their own calls (no call at all: 0 * 0 - 0 == 0)
   for (uint64_t j = 0; j < P; j++) {
      const uint64_t n = totals[3 * j], sx = totals[3 * j + 1], sq = totals[3 * j + 2];
      keep[j] = (keep[j] && n * sq - sx * sx != 0) ? 1 : 0;
   }
   auto above = [&](uint64_t i, uint64_t j) {
      const uint64_t d = j - i - 1;
      return (d >> 5) < words && ((bits[i * words + (d >> 5)] >> (d & 31)) & 1u);
   };
   for (uint64_t c0 = 0; c0 < P;) {
      uint64_t c1 = c0 + 1;
      while (chrom ? (c1 < P && chrom[c1] == chrom[c0]) : c1 < P) c1++;
      const uint64_t L = c1 - c0;
      // A pair inside the previous window has been examined there unless one of the two was already dropped, and a dropped SNP stays
      // dropped: among the survivors no such pair is above the threshold.  Only the pairs whose j is new to this window can fire.
      uint64_t prev_end = 0;
      for (uint64_t o = 0;; o += step) {
         const uint64_t end = std::min<uint64_t>(o + window, L);
         for (uint64_t i = o; i < end; i++) {
            const uint64_t gi = c0 + i;
            if (!keep[gi]) continue;
            for (uint64_t j = std::max(i + 1, prev_end); j < end; j++) {
               const uint64_t gj = c0 + j;
               if (!keep[gj] || !above(gi, gj)) continue;
               if (maf[gi] < maf[gj]) {
                  keep[gi] = 0;
                  break;
               }
               keep[gj] = 0;
            }
         }
         prev_end = end;
         if (end >= L) break;
      }
      c0 = c1;
   }
   uint64_t kept = 0;
   for (uint64_t j = 0; j < P; j++) kept += keep[j];
   return kept;
}

} // namespace fpca

extern "C" int fpca_ld_band(fpca_ctx *ctx, uint64_t snp0, uint64_t nsnp, uint32_t span, double *r2)
{
   return guarded([&] {
      ld_refuse(ctx, "fpca_ld_band", false);
      if (!r2) throw Error(FPCA_EINVAL, "bad argument to fpca_ld_band (r2 is NULL)");
      if (span == 0) throw Error(FPCA_EINVAL, "fpca_ld_band: span = 0; the band holds the pairs 1 .. span apart");
      if (nsnp == 0 || snp0 >= ctx->P_g || nsnp > ctx->P_g - snp0)
         throw Error(FPCA_EINVAL, "fpca_ld_band: SNPs [" + std::to_string(snp0) + ", " + std::to_string(snp0) + " + " + std::to_string(nsnp) +
                                      ") are not a non-empty range of this context's " + std::to_string(ctx->P_g) + " SNPs");
      if (nsnp > LD_BAND_LIMIT / sizeof(double) / span)
         throw Error(FPCA_EINVAL, "fpca_ld_band: a band of " + std::to_string(nsnp) + " SNPs x " + std::to_string(span) + " doubles is over the limit of " +
                                      std::to_string(LD_BAND_LIMIT) + " bytes (" + std::to_string(LD_BAND_LIMIT / sizeof(double) / span) +
                                      " SNPs at this span); call it range by range");
      const size_t count = (size_t)nsnp * span;
      HIP_CHECK(hipSetDevice(ctx->device));
      LdBufs s;
      ld_make_totals(ctx, s, "fpca_ld_band", snp0, nsnp);
      DevMem<double> d_r2(count, "fpca_ld_band", "the band of r2");
      HIP_CHECK(hipMemsetAsync(d_r2.p, 0xFF, count * sizeof(double), ctx->stream)); // (a NaN pattern; the host rewrites what no pair owns)
      kern::ld_band(ctx->d_packed, ctx->pitch, s.d_tot.p, (uint32_t)(ctx->N_pad - ctx->N), snp0, nsnp, snp0 + nsnp, span, d_r2.p, nullptr, 0, 0.0,
                    ld_force_general(), ctx->stream);
      HIP_CHECK(hipMemcpyAsync(r2, d_r2.p, count * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
      HIP_CHECK(hipStreamSynchronize(ctx->stream));
      const double nan = std::nan("");
      for (uint64_t i = nsnp > span ? nsnp - span : 0; i < nsnp; i++) // positions past the last SNP of the range
         for (uint64_t d = nsnp - i; d <= span; d++) r2[i * span + d - 1] = nan;
   });
}

extern "C" int fpca_ld_prune(fpca_ctx *ctx, const uint32_t *chrom, uint32_t window, uint32_t step, double r2, uint8_t *keep, uint64_t *n_kept)
{
   return guarded([&] {
      ld_refuse(ctx, "fpca_ld_prune", true);
      if (!keep) throw Error(FPCA_EINVAL, "bad argument to fpca_ld_prune (keep is NULL)");
      ld_check_window("fpca_ld_prune", window, step);
      if (std::isnan(r2) || r2 < 0 || r2 > 1) throw Error(FPCA_EINVAL, "fpca_ld_prune: the threshold r2 = " + std::to_string(r2) + " is not in [0, 1]");
      if (ctx->P_g > 0xFFFFFFFFull) throw Error(FPCA_EINVAL, "fpca_ld_prune: this context has " + std::to_string(ctx->P_g) + " SNPs; at most 2^32 - 1");
      HIP_CHECK(hipSetDevice(ctx->device));
      ensure_stats(ctx);
      const uint64_t P = ctx->P_g;
      // no pair is further apart than the window allows, or than the matrix is long
      const uint32_t span = (uint32_t)std::min<uint64_t>(window - 1, std::max<uint64_t>(P - 1, 1)), words = (span + 31) / 32;
      uint64_t slab = std::max<uint64_t>(LD_BITS_SLAB / (words * sizeof(uint32_t)) / LD_TILE * LD_TILE, LD_TILE);
      if (const char *v = FPCA_TEST_ENV("FPCA_LD_SLAB_ROWS"))
         if (std::atoll(v) > 0) slab = (uint64_t)std::atoll(v);
      slab = std::min(slab, P);
      const auto t0 = std::chrono::steady_clock::now();
      LdBufs s;
      ld_make_totals(ctx, s, "fpca_ld_prune", 0, ctx->P_g);
      ld_alloc_bits(ctx, s, "fpca_ld_prune", slab, words);
      std::vector<uint32_t> h_tot(P * 4), h_bits(P * words);
      std::vector<double> maf(P);
      HIP_CHECK(hipMemcpyAsync(h_tot.data(), s.d_tot.p, P * 4 * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
      HIP_CHECK(hipMemcpyAsync(maf.data(), ctx->d_mean, P * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
      for (uint64_t b = 0; b < P; b += slab) {
         const uint64_t nb = std::min(slab, P - b);
         HIP_CHECK(hipMemsetAsync(s.d_bits.p, 0, nb * words * sizeof(uint32_t), ctx->stream));
         kern::ld_band(ctx->d_packed, ctx->pitch, s.d_tot.p, (uint32_t)(ctx->N_pad - ctx->N), b, nb, P, span, nullptr, s.d_bits.p, words, r2, ld_force_general(),
                       ctx->stream);
         HIP_CHECK(hipMemcpyAsync(h_bits.data() + b * words, s.d_bits.p, nb * words * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
      }
      HIP_CHECK(hipStreamSynchronize(ctx->stream));
      const auto t1 = std::chrono::steady_clock::now();
      std::vector<uint64_t> totals(P * 3);
      for (uint64_t j = 0; j < P; j++) {
         totals[3 * j] = ctx->N_pad - h_tot[4 * j + 2]; // calls = sample slots - (missing calls + pad samples)
         totals[3 * j + 1] = h_tot[4 * j];
         totals[3 * j + 2] = h_tot[4 * j + 1];
         // maf exactly as snp_qc_rule computes it from K1's mean
         const double p = maf[j] / 2.0;
         maf[j] = (ctx->h_nmiss[j] >= ctx->N || std::isnan(p)) ? 0.0 : std::min(p, 1.0 - p);
      }
      const uint64_t kept = ld_prune_rule(h_bits.data(), words, P, window, step, totals.data(), maf.data(), chrom, keep);
      if (n_kept) *n_kept = kept;
      if (FPCA_TEST_ENV("FPCA_LD_TIMING")) { // (scripts/ld_prune_measure.py: the two halves of the call)
         const auto t2 = std::chrono::steady_clock::now();
         std::fprintf(stderr, "fpca_ld_prune: device (totals, %llu slab(s) of the bitmap kernel, %.1f MB downloaded) %.3f ms, host rule %.3f ms\n",
                      (unsigned long long)((P + slab - 1) / slab), (double)(P * words * 4) / 1e6,
                      std::chrono::duration<double, std::milli>(t1 - t0).count(), std::chrono::duration<double, std::milli>(t2 - t1).count());
      }
   });
}

extern "C" int fpca_debug_ld_prune_rule(const uint32_t *bits, uint64_t P, uint32_t window, uint32_t step, const uint64_t *totals, const double *maf,
                                        const uint32_t *chrom, uint8_t *keep, uint64_t *n_kept)
{
   return guarded([&] {
      if (!bits || !totals || !maf || !keep) throw Error(FPCA_EINVAL, "bad argument to fpca_debug_ld_prune_rule");
      ld_check_window("fpca_debug_ld_prune_rule", window, step);
      const uint64_t kept = ld_prune_rule(bits, (window - 1 + 31) / 32, P, window, step, totals, maf, chrom, keep);
      if (n_kept) *n_kept = kept;
   });
}

extern "C" int fpca_bench_ld(fpca_ctx *ctx, uint32_t span, int reps, double *ms, double *macs)
{
   return guarded([&] {
      ld_refuse(ctx, "fpca_bench_ld", false);
      if (!ms || reps < 1 || span == 0) throw Error(FPCA_EINVAL, "bad argument to fpca_bench_ld");
      HIP_CHECK(hipSetDevice(ctx->device));
      const uint64_t P = ctx->P_g;
      const uint32_t words = (span + 31) / 32, npad = (uint32_t)(ctx->N_pad - ctx->N);
      LdBufs s;
      ld_make_totals(ctx, s, "fpca_bench_ld", 0, ctx->P_g);
      ld_alloc_bits(ctx, s, "fpca_bench_ld", P, words);
      DevEvent e0("fpca_bench_ld"), e1("fpca_bench_ld");
      HIP_CHECK(hipMemsetAsync(s.d_bits.p, 0, (size_t)P * words * sizeof(uint32_t), ctx->stream));
      kern::ld_band(ctx->d_packed, ctx->pitch, s.d_tot.p, npad, 0, P, P, span, nullptr, s.d_bits.p, words, 0.05, ld_force_general(), ctx->stream);
      for (int r = 0; r < reps; r++) {
         HIP_CHECK(hipEventRecord(e0, ctx->stream));
         kern::ld_band(ctx->d_packed, ctx->pitch, s.d_tot.p, npad, 0, P, P, span, nullptr, s.d_bits.p, words, 0.05, ld_force_general(), ctx->stream);
         HIP_CHECK(hipEventRecord(e1, ctx->stream));
         HIP_CHECK(hipEventSynchronize(e1));
         ms[r] = elapsed_ms(e0, e1);
      }
      if (macs) { // the kernel's own wave-level decisions, replayed on the host
         std::vector<uint32_t> h_tot(P * 4);
         HIP_CHECK(hipMemcpy(h_tot.data(), s.d_tot.p, P * 4 * sizeof(uint32_t), hipMemcpyDeviceToHost));
         auto clean = [&](uint64_t a) {
            for (uint64_t l = 0; l < 32; l++)
               if (h_tot[4 * std::min(a + l, P - 1) + 2] != npad) return false;
            return true;
         };
         const bool force = ld_force_general();
         const uint64_t nj = ld_nj(span);
         double mfma = 0;
         for (uint64_t tI = 0; tI * LD_TILE < P; tI++)
            for (uint64_t x = 0; x < nj; x++)
               for (int w = 0; w < 4; w++) {
                  const uint64_t ia = tI * LD_TILE + (uint64_t)(w >> 1) * 32, ja = (tI + x) * LD_TILE + (uint64_t)(w & 1) * 32;
                  if (ia >= P || ja >= P || ja + 31 <= ia || (ja > ia + 31 && ja - (ia + 31) > span)) continue;
                  mfma += (force || !clean(ia) || !clean(ja)) ? 6.0 : 1.0;
               }
         *macs = mfma * (double)(ctx->pitch / 128) * 16.0 * 32768.0;
      }
   });
}
