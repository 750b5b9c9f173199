// king_rel.hip -- the KING relationship table: fpca_king_counts_block / fpca_king_related / fpca_king_cutoff_shared / fpca_king_classify
// (include/fpca.h "Kinship"), fpca_bench_king_rel.
//
// king.hip gives one number per pair, phi.  Here a pair also gets the integers KING's own table rests on: the SNPs called in both samples
// (shared), those at which the two hold opposite homozygotes (ibs0), those at which both are heterozygous (hethet), and het_i, het_j, D of
// king.hip -- from SEVEN int8 products per pair instead of five: the planes of ld_planes.hpp (x, q, e) and one more, h (1 at a
// heterozygous call; v_perm table 0x00010000).  With m = 1 - e, S = 4 pitch slots (pad included), Sx / Sq / Se the padded totals:
//      n     = sum m_i m_j = S - Se_i - Se_j + e_i.e_j
//      xm_i  = sum x_i m_j = Sx_i - x_i.e_j          mx_j = Sx_j - e_i.x_j          (q likewise; het_i, het_j, D as in king.hip)
//      hh    = h_i.h_j
//      ss    = x_i.x_j - xm_i - mx_j + n       s = x - m in {-1, 0, 1}: +1 for 2/2 and 0/0, -1 for 2/0 and 0/2, 0 where either is het or missing
//      tt    = n - het_i - het_j + hh          both called and both homozygous
//      ibs0  = (tt - ss) / 2                   always even, never negative
//   k_king_rel    the geometry of k_king: one workgroup (4 waves, 2 x 2) per pair of 64-sample tiles, a wave owns one 32 x 32 block of pairs
//                 and SEVEN accumulator planes (x.x, x.e, e.x, q.e, e.q, e.e, h.h: 112 registers); operands straight from the sample-major
//                 copy as 16-byte loads, the next chunk's in flight under this chunk's MFMAs; no LDS, no barrier.  A wave whose two blocks
//                 hold no missing call multiplies x.x and h.h only: there e.e = npad and the mixed planes are 0.
//                 BLOCK: counts[ni][nj][6] (shared, ibs0, hethet, het_i, het_j, D) and, optionally, phi[ni][nj] over any rectangle.
//                 PAIRS: the strict upper triangle; a pair with phi > thr AND shared >= min_shared whose samples are both in `keep` is
//                 appended (i, j, phi, the six counts) through atomicAdd on one counter, stored only below the capacity.
// phi is formed exactly as in k_king -- the same int64 numerator and denominator, one fp64 divide -- so it equals fpca_king_block bit for bit.
// The inner loop is this file's own: ld_planes.hpp, ld_band.hip and king.hip are not touched.
#include <algorithm>
#include <cmath>
#include <limits>

#include "ctx.hpp"
#include "launch_check.hpp"
#include "ld_planes.hpp"

using namespace fpca;

namespace {

constexpr int REL_TILE = 64;                         // samples per workgroup tile side (2 waves x 32)
constexpr uint64_t REL_MAX_P = 1ull << 28;           // 4 P_pad < 2^31: every sum fits the int32 accumulators
constexpr uint64_t REL_BLOCK_LIMIT = 1ull << 30;     // bytes of an fpca_king_counts_block buffer
constexpr uint64_t REL_LAUNCH_PAIRS = 1ull << 18;    // tile pairs of one launch
constexpr uint64_t REL_CUTOFF_CAP = 1ull << 26;      // pairs fpca_king_cutoff_shared keeps room for
constexpr int REL_BLOCK = 0, REL_PAIRS = 1;
constexpr int REL_NCOUNT = 6;                        // shared, ibs0, hethet, het_i, het_j, D
constexpr int XX = 0, XE = 1, EX = 2, QE = 3, EQ = 4, EE = 5, HH = 6;

// ld_decode of ld_planes.hpp plus the plane h (raw code 2 -> 1); the fast path needs x and h only
template <bool GENERAL>
__device__ __forceinline__ void rel_decode(uint32_t w, v4i &x, v4i &q, v4i &e, v4i &h)
{
#pragma unroll
   for (int s = 0; s < 4; s++) {
      const uint32_t sel = (w >> (2 * s)) & 0x03030303u;
      x[s] = (int)__builtin_amdgcn_perm(0u, 0x00010002u, sel);
      h[s] = (int)__builtin_amdgcn_perm(0u, 0x00010000u, sel);
      if (GENERAL) {
         q[s] = (int)__builtin_amdgcn_perm(0u, 0x00010004u, sel);
         e[s] = (int)__builtin_amdgcn_perm(0u, 0x00000100u, sel);
      }
   }
}

// ld_products of ld_planes.hpp with seven planes: acc[XX] += x.x, acc[HH] += h.h and, GENERAL, the four mixed planes and e.e
template <bool GENERAL>
__device__ __forceinline__ void rel_products(const uint4 *__restrict__ pa, const uint4 *__restrict__ pb, uint32_t nchunks, v16i (&acc)[7])
{
   uint4 a[4], b[4];
#pragma unroll
   for (int p = 0; p < 4; p++) {
      a[p] = pa[p];
      b[p] = pb[p];
   }
   for (uint32_t c = 0; c < nchunks; c++) {
      // the next chunk's 128 bytes per lane are in flight under this chunk's MFMAs (the last iteration re-reads its own chunk)
      const uint32_t cn = c + 1 < nchunks ? c + 1 : c;
      uint4 an[4], bn[4];
#pragma unroll
      for (int p = 0; p < 4; p++) {
         an[p] = pa[(size_t)cn * 8 + p];
         bn[p] = pb[(size_t)cn * 8 + p];
      }
#pragma unroll
      for (int p = 0; p < 4; p++) {
         const uint32_t wa[4] = {a[p].x, a[p].y, a[p].z, a[p].w}, wb[4] = {b[p].x, b[p].y, b[p].z, b[p].w};
#pragma unroll
         for (int d = 0; d < 4; d++) {
            v4i xa, qa, ea, ha, xb, qb, eb, hb;
            rel_decode<GENERAL>(wa[d], xa, qa, ea, ha);
            rel_decode<GENERAL>(wb[d], xb, qb, eb, hb);
            acc[XX] = __builtin_amdgcn_mfma_i32_32x32x32_i8(xa, xb, acc[XX], 0, 0, 0);
            acc[HH] = __builtin_amdgcn_mfma_i32_32x32x32_i8(ha, hb, acc[HH], 0, 0, 0);
            if (GENERAL) {
               acc[XE] = __builtin_amdgcn_mfma_i32_32x32x32_i8(xa, eb, acc[XE], 0, 0, 0);
               acc[EX] = __builtin_amdgcn_mfma_i32_32x32x32_i8(ea, xb, acc[EX], 0, 0, 0);
               acc[QE] = __builtin_amdgcn_mfma_i32_32x32x32_i8(qa, eb, acc[QE], 0, 0, 0);
               acc[EQ] = __builtin_amdgcn_mfma_i32_32x32x32_i8(ea, qb, acc[EQ], 0, 0, 0);
               acc[EE] = __builtin_amdgcn_mfma_i32_32x32x32_i8(ea, eb, acc[EE], 0, 0, 0);
            }
         }
      }
#pragma unroll
      for (int p = 0; p < 4; p++) {
         a[p] = an[p];
         b[p] = bn[p];
      }
   }
}

// workgroup w -> (tI, tJ) = (w / ntj, w % ntj): tile tI holds samples [i0 + 64 tI, ...), tile tJ samples [j0 + 64 tJ, ...)
template <int MODE>
__global__ __launch_bounds__(256, 2) void k_king_rel(const uint8_t *__restrict__ packed, size_t pitch, const uint32_t *__restrict__ tot, uint32_t npad,
                                                     uint64_t nrec, uint64_t i0, uint64_t iend, uint64_t j0, uint64_t jend, uint32_t ntj,
                                                     int force_general, uint32_t *__restrict__ counts, double *__restrict__ phi,
                                                     const uint8_t *__restrict__ keep, double thr, uint32_t min_shared, uint64_t cap,
                                                     unsigned long long *__restrict__ count, uint32_t *__restrict__ out_i,
                                                     uint32_t *__restrict__ out_j, double *__restrict__ out_phi, uint32_t *__restrict__ out_counts)
{
   const uint64_t tI = blockIdx.x / ntj, tJ = blockIdx.x % ntj;
   const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, li = lane & 31, kh = lane >> 5;
   // this wave's 32 x 32 block of pairs: samples ia .. ia + 31 (MFMA operand A, output rows) x ja .. ja + 31 (operand B, output columns)
   const uint64_t ia = i0 + tI * REL_TILE + (uint64_t)(wave >> 1) * 32, ja = j0 + tJ * REL_TILE + (uint64_t)(wave & 1) * 32;
   // nothing to do (wave-uniform; the kernel has no barrier): the block lies past the range, or (PAIRS) wholly on or below the diagonal
   if (ia >= iend || ja >= jend) return;
   if (MODE == REL_PAIRS && ja + 31 <= ia) return;
   // records past the last one are read as the last one (their pairs are dropped in the epilogue): no load leaves [0, nrec)
   const uint64_t ra = ia + li < nrec ? ia + li : nrec - 1, rb = ja + li < nrec ? ja + li : nrec - 1;
   const uint4 ta = reinterpret_cast<const uint4 *>(tot)[ra], tb = reinterpret_cast<const uint4 *>(tot)[rb]; // (sum x, sum x^2, sum e, -)
   const bool general = force_general || __builtin_amdgcn_ballot_w64(ta.z != npad || tb.z != npad) != 0ull;
   const uint4 *pa = reinterpret_cast<const uint4 *>(packed + ra * pitch) + kh * 4;
   const uint4 *pb = reinterpret_cast<const uint4 *>(packed + rb * pitch) + kh * 4;
   const uint32_t nchunks = (uint32_t)(pitch / 128);
   v16i acc[7];
#pragma unroll
   for (int m = 0; m < 7; m++)
#pragma unroll
      for (int r = 0; r < 16; r++) acc[m][r] = 0;
   if (general) {
      rel_products<true>(pa, pb, nchunks, acc);
   } else {
      // e is 1 at the pad SNPs of both sides only, where x = q = 0: the mixed products stay 0 and e.e is the pad count
      rel_products<false>(pa, pb, nchunks, acc);
#pragma unroll
      for (int r = 0; r < 16; r++) acc[EE][r] = (int)npad;
   }
   // Epilogue: the identities at the head of this file, exact in int64; phi as in k_king, ONE fp64 divide of two converted integers.
   const int64_t S = (int64_t)(4 * pitch);
   const uint64_t j = ja + li;
   const bool keep_j = MODE == REL_PAIRS && j < jend && (!keep || keep[j]);
#pragma unroll
   for (int r = 0; r < 16; r++) {
      const int row = (r & 3) + 8 * (r >> 2) + 4 * kh; // v_mfma_i32_32x32x32_i8: register r of lane (li, kh) is D[row][li]
      const uint64_t i = ia + row;
      if (i >= iend || j >= jend) continue;
      if (MODE == REL_PAIRS && (j <= i || !keep_j || (keep && !keep[i]))) continue;
      const uint4 ti = reinterpret_cast<const uint4 *>(tot)[i];
      const int64_t n = S - (int64_t)ti.z - (int64_t)tb.z + acc[EE][r];
      const int64_t xmi = (int64_t)ti.x - acc[XE][r], mxj = (int64_t)tb.x - acc[EX][r];
      const int64_t qi = (int64_t)ti.y - acc[QE][r], qj = (int64_t)tb.y - acc[EQ][r];
      const int64_t het_i = 2 * xmi - qi, het_j = 2 * mxj - qj;
      const int64_t D = qi + qj - 2 * (int64_t)acc[XX][r], hmin = het_i < het_j ? het_i : het_j;
      const int64_t hh = acc[HH][r];
      const int64_t ss = (int64_t)acc[XX][r] - xmi - mxj + n, tt = n - het_i - het_j + hh;
      const int64_t ibs0 = (tt - ss) / 2;
      const double v = hmin == 0 ? __builtin_nan("") : (double)(2 * hmin - D) / (double)(4 * hmin);
      uint32_t *dst;
      if (MODE == REL_BLOCK) {
         const size_t at = (size_t)(i - i0) * (jend - j0) + (j - j0);
         if (phi) phi[at] = v;
         dst = counts + at * REL_NCOUNT;
      } else {
         if (!(v > thr) || n < (int64_t)min_shared) continue;
         const unsigned long long slot = atomicAdd(count, 1ull);
         if (slot >= cap) continue;
         out_i[slot] = (uint32_t)i;
         out_j[slot] = (uint32_t)j;
         out_phi[slot] = v;
         dst = out_counts + (size_t)slot * REL_NCOUNT;
      }
      dst[0] = (uint32_t)n;
      dst[1] = (uint32_t)ibs0;
      dst[2] = (uint32_t)hh;
      dst[3] = (uint32_t)het_i;
      dst[4] = (uint32_t)het_j;
      dst[5] = (uint32_t)D;
   }
}

// what every entry point refuses (before any device work): the refusals of king.hip, word for word
void rel_refuse(const fpca_ctx *c, const char *fn)
{
   if (!c) throw Error(FPCA_EINVAL, std::string("bad argument to ") + fn + " (NULL context)");
   if (c->dense)
      throw Error(FPCA_EINVAL, std::string(fn) + ": this context holds a dense matrix; kinship is computed from the packed genotypes (fpca_create, "
                                                 "fpca_create_from_bed, synthetic)");
   if (c->masked())
      throw Error(FPCA_EINVAL, std::string(fn) + ": a sample mask is set (fpca_set_sample_mask); clear it and pass the mask as `keep` instead");
   if (c->multi() || (c->rank_known && c->nranks > 1))
      throw Error(FPCA_EINVAL, std::string(fn) + ": this context is one shard of several (a communicator, an all-reduce hook or fpca_set_rank with "
                                                 "more than one rank); kinship sums over all SNPs -- compute it on a single context");
   if (c->P_g > REL_MAX_P)
      throw Error(FPCA_EINVAL, std::string(fn) + ": " + std::to_string(c->P_g) + " SNPs; above 2^28 = 268,435,456 the sums no longer fit 32 bits");
   if (c->N > 0xFFFFFFFFull) throw Error(FPCA_EINVAL, std::string(fn) + ": this context has " + std::to_string(c->N) + " samples; at most 2^32 - 1");
}

bool rel_force_general()
{
   const char *v = FPCA_TEST_ENV("FPCA_KING_FORCE_GENERAL");
   return v && *v && *v != '0';
}

// device buffers of one call
struct RelBufs {
   DevMem<uint8_t> d_smp, d_keep; // the sample-major copy [N_pad][pitch]; keep [N]
   size_t pitch = 0;
   uint32_t npad = 0;
   DevMem<uint32_t> d_tot, d_i, d_j, d_counts;
   DevMem<double> d_phi;
   DevMem<unsigned long long> d_count;
   // the pair list of `slots` entries and its counter
   void alloc_pairs(size_t slots, const char *fn)
   {
      d_i = DevMem<uint32_t>(slots, fn, "the pair list (i)");
      d_j = DevMem<uint32_t>(slots, fn, "the pair list (j)");
      d_phi = DevMem<double>(slots, fn, "the pair list (phi)");
      d_counts = DevMem<uint32_t>(slots * REL_NCOUNT, fn, "the pair list (counts)");
      d_count = DevMem<unsigned long long>(1, fn, "the pair counter");
   }
};

// the sample-major operand and its per-sample totals, enqueued on the context's stream (as king.hip makes them)
void rel_make_operand(fpca_ctx *c, RelBufs &s, const char *fn)
{
   s.pitch = (size_t)round_up(c->P_pad / 4, 128);
   s.npad = (uint32_t)(4 * s.pitch - c->P_g);
   const size_t need = (size_t)c->N_pad * s.pitch;
   char detail[96];
   std::snprintf(detail, sizeof(detail), "%llu samples x %llu bytes", (unsigned long long)c->N_pad, (unsigned long long)s.pitch);
   s.d_smp = DevMem<uint8_t>(need, fn, "sample-major copy", 0, detail, c->device);
   HIP_CHECK(hipMemsetAsync(s.d_smp.p, PAD_BYTE, need, c->stream));
   kern::transpose_packed(c->d_packed, c->pitch, c->N_pad, c->P_pad, s.d_smp.p, s.pitch, c->stream, false);
   s.d_tot = DevMem<uint32_t>(c->N * 4, fn, "the per-sample totals");
   kern::ld_totals(s.d_smp.p, s.pitch, c->N, s.d_tot.p, c->stream);
}

void rel_launch(int mode, const fpca_ctx *c, const RelBufs &s, uint64_t i0, uint64_t iend, uint64_t j0, uint64_t jend, uint32_t *counts, double *phi,
                double thr, uint32_t min_shared, uint64_t cap)
{
   const uint64_t nti = (iend - i0 + REL_TILE - 1) / REL_TILE, ntj = (jend - j0 + REL_TILE - 1) / REL_TILE, wgs = nti * ntj;
   if (!wgs) return;
   if (wgs > 0x7FFFFFFFull || ntj > 0xFFFFFFFFull) throw Error(FPCA_EINVAL, "kinship: " + std::to_string(wgs) + " tile pairs exceed one launch");
   if (mode == REL_BLOCK)
      hipLaunchKernelGGL(k_king_rel<REL_BLOCK>, dim3((unsigned)wgs), dim3(256), 0, c->stream, s.d_smp.p, s.pitch, s.d_tot.p, s.npad, c->N, i0, iend, j0,
                         jend, (uint32_t)ntj, (int)rel_force_general(), counts, phi, s.d_keep.p, thr, min_shared, cap, s.d_count.p, s.d_i.p, s.d_j.p,
                         s.d_phi.p, s.d_counts.p);
   else
      hipLaunchKernelGGL(k_king_rel<REL_PAIRS>, dim3((unsigned)wgs), dim3(256), 0, c->stream, s.d_smp.p, s.pitch, s.d_tot.p, s.npad, c->N, i0, iend, j0,
                         jend, (uint32_t)ntj, (int)rel_force_general(), counts, phi, s.d_keep.p, thr, min_shared, cap, s.d_count.p, s.d_i.p, s.d_j.p,
                         s.d_phi.p, s.d_counts.p);
   launch_check();
}

// the strict upper triangle in slabs of row tiles: slab [ta, tb) x column tiles [ta, nt); the blocks below the diagonal return at once
void rel_triangle(const fpca_ctx *c, const RelBufs &s, double thr, uint32_t min_shared, uint64_t cap)
{
   const uint64_t N = c->N, nt = (N + REL_TILE - 1) / REL_TILE;
   uint64_t forced = 0;
   if (const char *v = FPCA_TEST_ENV("FPCA_KING_SLAB_ROWS"))
      if (std::atoll(v) > 0) forced = ((uint64_t)std::atoll(v) + REL_TILE - 1) / REL_TILE;
   for (uint64_t ta = 0; ta < nt;) {
      const uint64_t rows = forced ? forced : std::max<uint64_t>(REL_LAUNCH_PAIRS / (nt - ta), 1), tb = std::min(ta + rows, nt);
      rel_launch(REL_PAIRS, c, s, ta * REL_TILE, std::min(tb * REL_TILE, N), ta * REL_TILE, N, nullptr, nullptr, thr, min_shared, cap);
      ta = tb;
   }
}

struct RelPair {
   uint32_t i, j;
   double phi;
   uint32_t counts[REL_NCOUNT];
};

// the pair pass: every pair i < j of kept samples with phi > thr and shared >= min_shared, sorted by (i, j), when no more than `cap`
// qualify; returns how many do
uint64_t rel_pair_pass(fpca_ctx *c, const char *fn, const uint8_t *keep, double thr, uint32_t min_shared, uint64_t cap, std::vector<RelPair> &out)
{
   const uint64_t N = c->N;
   cap = std::min<uint64_t>(cap, N * (N - 1) / 2);
   HIP_CHECK(hipSetDevice(c->device));
   RelBufs s;
   rel_make_operand(c, s, fn);
   if (keep) {
      s.d_keep = DevMem<uint8_t>(N, fn, "the sample mask");
      HIP_CHECK(hipMemcpyAsync(s.d_keep.p, keep, N, hipMemcpyHostToDevice, c->stream));
   }
   s.alloc_pairs((size_t)std::max<uint64_t>(cap, 1), fn);
   HIP_CHECK(hipMemsetAsync(s.d_count.p, 0, sizeof(unsigned long long), c->stream));
   rel_triangle(c, s, thr, min_shared, cap);
   unsigned long long found = 0;
   HIP_CHECK(hipMemcpyAsync(&found, s.d_count.p, sizeof(found), hipMemcpyDeviceToHost, c->stream));
   HIP_CHECK(hipStreamSynchronize(c->stream));
   out.clear();
   if (found > cap || found == 0) return found;
   std::vector<uint32_t> hi(found), hj(found), hc(found * REL_NCOUNT);
   std::vector<double> hp(found);
   HIP_CHECK(hipMemcpy(hi.data(), s.d_i.p, found * sizeof(uint32_t), hipMemcpyDeviceToHost));
   HIP_CHECK(hipMemcpy(hj.data(), s.d_j.p, found * sizeof(uint32_t), hipMemcpyDeviceToHost));
   HIP_CHECK(hipMemcpy(hp.data(), s.d_phi.p, found * sizeof(double), hipMemcpyDeviceToHost));
   HIP_CHECK(hipMemcpy(hc.data(), s.d_counts.p, found * REL_NCOUNT * sizeof(uint32_t), hipMemcpyDeviceToHost));
   out.resize(found);
   for (uint64_t k = 0; k < found; k++) {
      out[k].i = hi[k];
      out[k].j = hj[k];
      out[k].phi = hp[k];
      std::copy(&hc[k * REL_NCOUNT], &hc[k * REL_NCOUNT] + REL_NCOUNT, out[k].counts);
   }
   std::sort(out.begin(), out.end(), [](const RelPair &a, const RelPair &b) { return a.i != b.i ? a.i < b.i : a.j < b.j; });
   return found;
}

} // namespace

extern "C" int fpca_king_counts_block(fpca_ctx *ctx, uint64_t i0, uint64_t ni, uint64_t j0, uint64_t nj, uint32_t *counts, double *phi)
{
   return guarded([&] {
      rel_refuse(ctx, "fpca_king_counts_block");
      if (!counts) throw Error(FPCA_EINVAL, "bad argument to fpca_king_counts_block (counts is NULL)");
      const uint64_t N = ctx->N;
      if (ni == 0 || nj == 0 || i0 >= N || ni > N - i0 || j0 >= N || nj > N - j0)
         throw Error(FPCA_EINVAL, "fpca_king_counts_block: samples [" + std::to_string(i0) + ", " + std::to_string(i0) + " + " + std::to_string(ni) +
                                      ") x [" + std::to_string(j0) + ", " + std::to_string(j0) + " + " + std::to_string(nj) +
                                      ") are not a non-empty rectangle of this context's " + std::to_string(N) + " samples");
      if (ni > REL_BLOCK_LIMIT / (REL_NCOUNT * sizeof(uint32_t)) / nj)
         throw Error(FPCA_EINVAL, "fpca_king_counts_block: a block of " + std::to_string(ni) + " x " + std::to_string(nj) + " x 6 counts is over the limit of " +
                                      std::to_string(REL_BLOCK_LIMIT) + " bytes; call it block by block");
      const size_t cells = (size_t)ni * nj;
      HIP_CHECK(hipSetDevice(ctx->device));
      RelBufs s;
      rel_make_operand(ctx, s, "fpca_king_counts_block");
      DevMem<uint32_t> d_counts(cells * REL_NCOUNT, "fpca_king_counts_block", "the block of counts");
      DevMem<double> d_phi;
      if (phi) d_phi = DevMem<double>(cells, "fpca_king_counts_block", "the block of coefficients");
      rel_launch(REL_BLOCK, ctx, s, i0, i0 + ni, j0, j0 + nj, d_counts.p, d_phi.p, 0.0, 0, 0);
      HIP_CHECK(hipMemcpyAsync(counts, d_counts.p, cells * REL_NCOUNT * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
      if (phi) HIP_CHECK(hipMemcpyAsync(phi, d_phi.p, cells * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
      HIP_CHECK(hipStreamSynchronize(ctx->stream));
   });
}

extern "C" int fpca_king_related(fpca_ctx *ctx, const uint8_t *keep, double thr, uint32_t min_shared, uint64_t max_pairs, uint32_t *i, uint32_t *j,
                                 double *phi, uint32_t *counts, uint64_t *n_pairs)
{
   return guarded([&] {
      rel_refuse(ctx, "fpca_king_related");
      if (!n_pairs || (max_pairs && (!i || !j || !phi || !counts))) throw Error(FPCA_EINVAL, "bad argument to fpca_king_related (a NULL output)");
      if (std::isnan(thr)) throw Error(FPCA_EINVAL, "fpca_king_related: the threshold is NaN");
      const uint64_t room = std::min<uint64_t>(max_pairs, ctx->N * (ctx->N - 1) / 2); // what the pass allocates and the caller's arrays must hold
      if (room > REL_BLOCK_LIMIT / (REL_NCOUNT * sizeof(uint32_t)))
         throw Error(FPCA_EINVAL, "fpca_king_related: room for " + std::to_string(room) + " pairs x 6 counts is over the limit of " +
                                      std::to_string(REL_BLOCK_LIMIT) + " bytes; pass a smaller max_pairs");
      std::vector<RelPair> pairs;
      const uint64_t found = rel_pair_pass(ctx, "fpca_king_related", keep, thr, min_shared, max_pairs, pairs);
      *n_pairs = found;
      if (found > max_pairs)
         throw Error(FPCA_ENOMEM, "fpca_king_related: " + std::to_string(found) + " pairs qualify, the arrays hold " + std::to_string(max_pairs) +
                                      "; call again with room for " + std::to_string(found));
      for (uint64_t k = 0; k < found; k++) {
         i[k] = pairs[k].i;
         j[k] = pairs[k].j;
         phi[k] = pairs[k].phi;
         std::copy(pairs[k].counts, pairs[k].counts + REL_NCOUNT, counts + k * REL_NCOUNT);
      }
   });
}

extern "C" int fpca_king_cutoff_shared(fpca_ctx *ctx, double thr, uint32_t min_shared, uint8_t *keep, uint64_t *n_kept)
{
   return guarded([&] {
      rel_refuse(ctx, "fpca_king_cutoff_shared");
      if (!keep) throw Error(FPCA_EINVAL, "bad argument to fpca_king_cutoff_shared (keep is NULL)");
      if (std::isnan(thr)) throw Error(FPCA_EINVAL, "fpca_king_cutoff_shared: the threshold is NaN");
      uint64_t cap = REL_CUTOFF_CAP;
      if (const char *v = FPCA_TEST_ENV("FPCA_KING_MAX_PAIRS"))
         if (std::atoll(v) > 0) cap = (uint64_t)std::atoll(v);
      std::vector<RelPair> pairs;
      const uint64_t found = rel_pair_pass(ctx, "fpca_king_cutoff_shared", keep, thr, min_shared, cap, pairs);
      if (found > cap)
         throw Error(FPCA_ENOMEM, "fpca_king_cutoff_shared: " + std::to_string(found) + " pairs qualify, the call keeps room for " + std::to_string(cap) +
                                      "; raise the threshold or thin the samples first (fpca_king_related lists them)");
      std::vector<uint32_t> pi(found), pj(found);
      for (uint64_t k = 0; k < found; k++) {
         pi[k] = pairs[k].i;
         pj[k] = pairs[k].j;
      }
      const uint64_t kept = king_cutoff_rule(pi.data(), pj.data(), found, ctx->N, keep);
      if (n_kept) *n_kept = kept;
   });
}

extern "C" int fpca_king_classify(uint64_t n_pairs, const double *phi, const uint32_t *counts, double po_ibs0, uint8_t *type)
{
   return guarded([&] {
      if (n_pairs && (!phi || !counts || !type)) throw Error(FPCA_EINVAL, "bad argument to fpca_king_classify (a NULL array)");
      if (!std::isfinite(po_ibs0) || po_ibs0 < 0) throw Error(FPCA_EINVAL, "fpca_king_classify: po_ibs0 is not a finite number >= 0");
      for (uint64_t k = 0; k < n_pairs; k++) {
         const double v = phi[k];
         const uint32_t shared = counts[k * REL_NCOUNT], ibs0 = counts[k * REL_NCOUNT + 1];
         uint8_t t = 0;
         if (std::isnan(v) || shared == 0)
            t = 255;
         else if (v > 0.354)
            t = 5;
         else if (v > 0.177)
            t = (double)ibs0 / (double)shared < po_ibs0 ? 1 : 2;
         else if (v > 0.0884)
            t = 3;
         else if (v > 0.0442)
            t = 4;
         type[k] = t;
      }
   });
}

extern "C" int fpca_bench_king_rel(fpca_ctx *ctx, int reps, double *ms, double *macs)
{
   return guarded([&] {
      rel_refuse(ctx, "fpca_bench_king_rel");
      if (!ms || reps < 1) throw Error(FPCA_EINVAL, "bad argument to fpca_bench_king_rel");
      HIP_CHECK(hipSetDevice(ctx->device));
      const uint64_t N = ctx->N, cap = 1ull << 20;
      const double thr = 0.0884;
      RelBufs s;
      rel_make_operand(ctx, s, "fpca_bench_king_rel");
      s.alloc_pairs(cap, "fpca_bench_king_rel");
      DevEvent e0("fpca_bench_king_rel"), e1("fpca_bench_king_rel");
      HIP_CHECK(hipMemsetAsync(s.d_count.p, 0, sizeof(unsigned long long), ctx->stream));
      rel_triangle(ctx, s, thr, 0, cap);
      for (int r = 0; r < reps; r++) {
         HIP_CHECK(hipMemsetAsync(s.d_count.p, 0, sizeof(unsigned long long), ctx->stream));
         HIP_CHECK(hipEventRecord(e0, ctx->stream));
         rel_triangle(ctx, s, thr, 0, cap);
         HIP_CHECK(hipEventRecord(e1, ctx->stream));
         HIP_CHECK(hipEventSynchronize(e1));
         ms[r] = elapsed_ms(e0, e1);
      }
      if (macs) { // the kernel's own wave-level decisions, replayed on the host
         std::vector<uint32_t> h_tot(N * 4);
         HIP_CHECK(hipMemcpy(h_tot.data(), s.d_tot.p, N * 4 * sizeof(uint32_t), hipMemcpyDeviceToHost));
         const uint64_t nb = (N + 31) / 32; // the waves' 32-sample blocks start at multiples of 32
         std::vector<uint8_t> clean(nb, 1);
         for (uint64_t b = 0; b < nb; b++)
            for (uint64_t l = 0; l < 32; l++)
               if (h_tot[4 * std::min(32 * b + l, N - 1) + 2] != s.npad) clean[b] = 0;
         const bool force = rel_force_general();
         double mfma = 0;
         for (uint64_t bi = 0; bi < nb; bi++)
            for (uint64_t bj = bi; bj < nb; bj++) mfma += (force || !clean[bi] || !clean[bj]) ? 7.0 : 2.0;
         *macs = mfma * (double)(s.pitch / 128) * 16.0 * 32768.0;
      }
   });
}
