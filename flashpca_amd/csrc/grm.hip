// grm.hip -- the genetic relationship matrix and a relatedness cutoff on it: fpca_grm_block / fpca_grm_tri / fpca_grm_pairs / fpca_grm_cutoff
// (include/fpca.h "Relationship matrix"), fpca_bench_grm.
//
// With z_is = t_s[code_is], the context's own table entry (make_lut: the standardised value at a call, 0 at a missing call, all four 0 for
// a SNP whose sd is <= 1e-9 or NaN), S_ij = sum_s z_is z_js and n_ij = the live SNPs (table not all zero) called in both samples, G_ij is
// S_ij / n_ij, S_ij / P_g or S_ij.  S is a Gram of real numbers: not k_king's exact-integer product but an FP64-MFMA kernel of its own.
//   operand       king.hip's: a row-major sample-major copy made for the call, N_pad rows of pitch = round_up(P_pad / 4, 128) bytes preset to
//                 PAD_BYTE.  k_grm_live marks the live SNPs (and counts them), k_grm_kill then turns every code of a non-live SNP into
//                 "missing" in the copy, so that n_ij is exactly the shared-call count of the copy and kern::ld_totals' third column its
//                 per-sample complement.
//   k_grm_dot     S on v_mfma_f64_16x16x4_f64.  One workgroup (4 waves, 2 x 2) per pair of 64-sample tiles, a wave owns a 32 x 32 block of
//                 pairs = four 16 x 16 accumulators (32 registers).  The MFMA's K = 4 is one packed byte: the lane with k = lane >> 4 takes
//                 field k of byte b of its sample's row and its operand is the table entry t_{4b+k}[code] itself, read from LDS, where the
//                 table of the current 128-byte chunk (512 SNPs x 4 doubles = 16 KB) is staged, double-buffered, one barrier per chunk; slots
//                 at or past P_g are staged as 0 without a read beyond the table.  Per byte and wave: four LDS reads, four MFMAs.  No
//                 atomics, no split along the SNPs: the order of the sum is fixed, a call is deterministic.  Records past the last are read
//                 as the last and dropped when S is stored.
//   k_grm_shared  n on v_mfma_i32_32x32x32_i8: the one product e.e of ld_planes.hpp's decode, n = 4 pitch - Se_i - Se_j + e_i.e_j.  A wave
//                 whose two blocks hold no missing call of a live SNP (Se == dead, the pad and non-live slots) stores the live count
//                 without a product.  Launched only when the divisor or the caller needs n.
//   k_grm_finish  the ONE fp64 divide (n == 0 tested: NaN) and the output: the rectangle, the packed triangle rows of the slab, or the pair
//                 list (atomicAdd on one 64-bit counter, a slot stored only below the capacity).
// S (fp64) and n (uint32) of a slab of rows, and the slab's output, live in device scratch.  The triangle is computed as j <= i (blocks wholly
// above the diagonal return at once); the pair list names a pair (i, j), i < j, from the cell (row j, column i).
#include <algorithm>
#include <cmath>
#include <limits>

#include "ctx.hpp"
#include "launch_check.hpp"
#include "ld_planes.hpp"

using namespace fpca;

namespace {

constexpr int GRM_TILE = 64;                         // samples per workgroup tile side (2 waves x 32)
constexpr uint64_t GRM_MAX_P = 1ull << 28;           // n_ij and the int32 accumulators of e.e
constexpr uint64_t GRM_BLOCK_LIMIT = 1ull << 30;     // bytes of an fpca_grm_block buffer
constexpr uint64_t GRM_LAUNCH_PAIRS = 1ull << 18;    // tile pairs of one launch
constexpr uint64_t GRM_SLAB_BYTES = 1ull << 28;      // S and n of one slab
constexpr uint64_t GRM_CUTOFF_CAP = 1ull << 26;      // pairs fpca_grm_cutoff keeps room for
constexpr int GRM_RECT = 0, GRM_TRI = 1, GRM_PAIRS = 2;
constexpr int GRM_CHUNK_SNPS = 512;                  // SNPs of one 128-byte chunk of a record

typedef double d4 __attribute__((ext_vector_type(4)));
typedef double d2 __attribute__((ext_vector_type(2)));

// one byte per 4 SNP slots of the copy: bits 2k, 2k + 1 set when SNP 4 b + k < P_g is NOT live; *n_live counts the live ones
__global__ __launch_bounds__(256) void k_grm_live(const double *__restrict__ lut, uint64_t P_g, size_t pitch, uint8_t *__restrict__ dead,
                                                   uint32_t *__restrict__ n_live)
{
   const uint64_t b = (uint64_t)blockIdx.x * 256 + threadIdx.x;
   uint32_t live = 0, mask = 0;
   if (b < pitch) {
#pragma unroll
      for (int k = 0; k < 4; k++) {
         const uint64_t s = 4 * b + k;
         if (s >= P_g) continue; // a pad slot: PAD_BYTE already reads as missing
         const d4 t = *reinterpret_cast<const d4 *>(lut + 4 * s);
         if (t.x != 0.0 || t.y != 0.0 || t.z != 0.0 || t.w != 0.0)
            live++;
         else
            mask |= 3u << (2 * k);
      }
      dead[b] = (uint8_t)mask;
   }
   // one atomic per wave
   for (int off = 32; off; off >>= 1) live += __shfl_down(live, off);
   if ((threadIdx.x & 63) == 0 && live) atomicAdd(n_live, live);
}

// every code of a non-live SNP becomes 01 (missing); 16 bytes per thread
__global__ __launch_bounds__(256) void k_grm_kill(uint8_t *__restrict__ smp, size_t pitch, uint64_t nrec, const uint8_t *__restrict__ dead)
{
   const uint64_t v = (uint64_t)blockIdx.x * 256 + threadIdx.x, per = pitch / 16;
   if (v >= nrec * per) return;
   const uint64_t rec = v / per, q = v % per;
   uint4 *p = reinterpret_cast<uint4 *>(smp + rec * pitch) + q;
   const uint4 m = reinterpret_cast<const uint4 *>(dead)[q];
   if ((m.x | m.y | m.z | m.w) == 0) return;
   uint4 w = *p;
   w.x = (w.x & ~m.x) | (m.x & 0x55555555u);
   w.y = (w.y & ~m.y) | (m.y & 0x55555555u);
   w.z = (w.z & ~m.z) | (m.z & 0x55555555u);
   w.w = (w.w & ~m.w) | (m.w & 0x55555555u);
   *p = w;
}

// workgroup w -> (tI, tJ) = (w / ntj, w % ntj): tile tI holds samples [i0 + 64 tI, ...), tile tJ samples [j0 + 64 tJ, ...).
// S[(i - i0) * ld + (j - j0)] for the cells of the launch's rectangle; TRI: blocks wholly above the diagonal (j > i everywhere) are skipped.
template <bool TRI>
__global__ __launch_bounds__(256, 2) void k_grm_dot(const uint8_t *__restrict__ packed, size_t pitch, const double *__restrict__ lut, uint64_t P_g,
                                                    uint64_t nrec, uint64_t i0, uint64_t iend, uint64_t j0, uint64_t jend, uint32_t ntj,
                                                    double *__restrict__ S, size_t ld)
{
   __shared__ double tab[2][GRM_CHUNK_SNPS * 4];
   const uint64_t tI = blockIdx.x / ntj, tJ = blockIdx.x % ntj;
   // the whole tile pair above the diagonal: nothing to do (uniform over the workgroup, before any barrier)
   if (TRI && j0 + tJ * GRM_TILE > i0 + tI * GRM_TILE + (GRM_TILE - 1)) return;
   const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, m = lane & 15, k = lane >> 4;
   // this wave's 32 x 32 block of pairs: samples ia .. ia + 31 (operand A, output rows) x ja .. ja + 31 (operand B, output columns)
   const uint64_t ia = i0 + tI * GRM_TILE + (uint64_t)(wave >> 1) * 32, ja = j0 + tJ * GRM_TILE + (uint64_t)(wave & 1) * 32;
   // a wave without work still stages the table and meets the barriers
   const bool active = ia < iend && ja < jend && !(TRI && ja > ia + 31);
   // records past the last one are read as the last one (their cells are dropped below): no load leaves [0, nrec)
   const uint8_t *row[4];
#pragma unroll
   for (int h = 0; h < 2; h++) {
      const uint64_t a = ia + 16 * h + m, b = ja + 16 * h + m;
      row[h] = packed + (a < nrec ? a : nrec - 1) * pitch;
      row[2 + h] = packed + (b < nrec ? b : nrec - 1) * pitch;
   }
   const uint32_t nchunks = (uint32_t)(pitch / 128), nsteps = nchunks * 8; // a step: 16 bytes of every record = 16 MFMA k-steps
   d4 acc[2][2];
#pragma unroll
   for (int a = 0; a < 2; a++)
#pragma unroll
      for (int b = 0; b < 2; b++) acc[a][b] = d4{0.0, 0.0, 0.0, 0.0};

   // the table of chunk c: 2048 doubles, 4 x 16 bytes per thread; slots at or past P_g are 0 and not read
   auto fetch = [&](uint32_t c, d2 (&t)[4]) {
#pragma unroll
      for (int u = 0; u < 4; u++) {
         const uint64_t e = (uint64_t)c * (GRM_CHUNK_SNPS * 4) + (uint64_t)u * 512 + 2 * tid;
         t[u] = (e >> 2) < P_g ? *reinterpret_cast<const d2 *>(lut + e) : d2{0.0, 0.0};
      }
   };
   auto stage = [&](int buf, const d2 (&t)[4]) {
#pragma unroll
      for (int u = 0; u < 4; u++) *reinterpret_cast<d2 *>(&tab[buf][u * 512 + 2 * tid]) = t[u];
   };
   {
      d2 t[4];
      fetch(0, t);
      stage(0, t);
   }
   uint4 cur[4];
#pragma unroll
   for (int r = 0; r < 4; r++) cur[r] = active ? *reinterpret_cast<const uint4 *>(row[r]) : uint4{0, 0, 0, 0};
   __syncthreads();
   for (uint32_t c = 0; c < nchunks; c++) {
      const int buf = c & 1;
      d2 tnext[4];
      const bool more = c + 1 < nchunks;
      if (more) fetch(c + 1, tnext);
      if (active) {
         for (uint32_t q = 0; q < 8; q++) {
            // the next 16 bytes of the four records are in flight under this step's MFMAs (the last step re-reads itself)
            const uint32_t st = c * 8 + q, sn = st + 1 < nsteps ? st + 1 : st;
            uint4 nxt[4];
#pragma unroll
            for (int r = 0; r < 4; r++) nxt[r] = reinterpret_cast<const uint4 *>(row[r])[sn];
            // entry [code] of SNP 4 b + k of the chunk, b = 16 q + 4 d + bb: tab[buf][(4 b + k) * 4 + code]
            const double *tq = &tab[buf][(q * 64 + k) * 4];
#pragma unroll
            for (int d = 0; d < 4; d++) {
               uint32_t w[4];
#pragma unroll
               for (int r = 0; r < 4; r++) {
                  const uint32_t x = d == 0 ? cur[r].x : d == 1 ? cur[r].y : d == 2 ? cur[r].z : cur[r].w;
                  w[r] = x >> (2 * k); // field k of byte bb is now at bits 8 bb, 8 bb + 1
               }
#pragma unroll
               for (int bb = 0; bb < 4; bb++) {
                  const double *tb = tq + (4 * d + bb) * 16;
                  double z[4];
#pragma unroll
                  for (int r = 0; r < 4; r++) z[r] = tb[(w[r] >> (8 * bb)) & 3u];
                  acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(z[0], z[2], acc[0][0], 0, 0, 0);
                  acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(z[0], z[3], acc[0][1], 0, 0, 0);
                  acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(z[1], z[2], acc[1][0], 0, 0, 0);
                  acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(z[1], z[3], acc[1][1], 0, 0, 0);
               }
            }
#pragma unroll
            for (int r = 0; r < 4; r++) cur[r] = nxt[r];
         }
      }
      // every wave has read buffer buf ^ 1 before the barrier that ended the previous chunk
      if (more) stage(buf ^ 1, tnext);
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
            if (i < iend) S[(size_t)(i - i0) * ld + (j - j0)] = acc[a][b][r];
         }
      }
}

// n[(i - i0) * ld + (j - j0)] = the live SNPs called in both samples; the geometry and the grid of k_grm_dot, no LDS, no barrier
template <bool TRI>
__global__ __launch_bounds__(256, 2) void k_grm_shared(const uint8_t *__restrict__ packed, size_t pitch, const uint32_t *__restrict__ tot,
                                                       const uint32_t *__restrict__ n_live, uint64_t nrec, uint64_t i0, uint64_t iend, uint64_t j0,
                                                       uint64_t jend, uint32_t ntj, int force_general, uint32_t *__restrict__ n, size_t ld)
{
   const uint64_t tI = blockIdx.x / ntj, tJ = blockIdx.x % ntj;
   const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, li = lane & 31, kh = lane >> 5;
   const uint64_t ia = i0 + tI * GRM_TILE + (uint64_t)(wave >> 1) * 32, ja = j0 + tJ * GRM_TILE + (uint64_t)(wave & 1) * 32;
   if (ia >= iend || ja >= jend) return;
   if (TRI && ja > ia + 31) return;
   const uint64_t ra = ia + li < nrec ? ia + li : nrec - 1, rb = ja + li < nrec ? ja + li : nrec - 1;
   const uint32_t slots = (uint32_t)(4 * pitch), dead = slots - *n_live; // the pad slots and the non-live SNPs: "missing" in every record
   const uint32_t ea = tot[4 * ra + 2], eb = tot[4 * rb + 2];            // sum e of the two records (kern::ld_totals)
   const bool general = force_general || __builtin_amdgcn_ballot_w64(ea != dead || eb != dead) != 0ull;
   v16i acc;
#pragma unroll
   for (int r = 0; r < 16; r++) acc[r] = (int)dead; // no missing call of a live SNP on either side: e.e is the dead count
   if (general) {
#pragma unroll
      for (int r = 0; r < 16; r++) acc[r] = 0;
      const uint4 *pa = reinterpret_cast<const uint4 *>(packed + ra * pitch) + kh * 4;
      const uint4 *pb = reinterpret_cast<const uint4 *>(packed + rb * pitch) + kh * 4;
      const uint32_t nchunks = (uint32_t)(pitch / 128);
      for (uint32_t c = 0; c < nchunks; c++) {
         uint4 a[4], b[4];
#pragma unroll
         for (int p = 0; p < 4; p++) {
            a[p] = pa[(size_t)c * 8 + p];
            b[p] = pb[(size_t)c * 8 + p];
         }
#pragma unroll
         for (int p = 0; p < 4; p++) {
            const uint32_t wa[4] = {a[p].x, a[p].y, a[p].z, a[p].w}, wb[4] = {b[p].x, b[p].y, b[p].z, b[p].w};
#pragma unroll
            for (int d = 0; d < 4; d++) {
               v4i xa, qa, e1, xb, qb, e2;
               ld_decode<true>(wa[d], xa, qa, e1);
               ld_decode<true>(wb[d], xb, qb, e2);
               acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(e1, e2, acc, 0, 0, 0);
            }
         }
      }
   }
   const uint64_t j = ja + li;
   if (j >= jend) return;
#pragma unroll
   for (int r = 0; r < 16; r++) {
      const int row = (r & 3) + 8 * (r >> 2) + 4 * kh; // v_mfma_i32_32x32x32_i8: register r of lane (li, kh) is D[row][li]
      const uint64_t i = ia + row;
      if (i >= iend) continue;
      // m = 1 - e: sum m_i m_j = slots - Se_i - Se_j + e_i.e_j
      n[(size_t)(i - i0) * ld + (j - j0)] = slots - tot[4 * i + 2] - eb + (uint32_t)acc[r];
   }
}

__device__ __forceinline__ double grm_value(double s, int divisor, uint32_t n, double P)
{
   if (divisor == FPCA_GRM_DIV_SHARED) return n == 0 ? __builtin_nan("") : s / (double)n;
   return divisor == FPCA_GRM_DIV_P ? s / P : s;
}

// one thread per cell (a, b) of the slab: sample i = i0 + a (row), j = j0 + b (column).  n may be null unless divisor is DIV_SHARED.
//   RECT   out[a * ld + b], every cell
//   TRI    j0 == 0; out[i (i + 1) / 2 + j - i0 (i0 + 1) / 2] and (out_n not null) the count likewise, j <= i
//   PAIRS  j0 == 0; the pair (j, i) for j < i, both kept, value > thr
template <int MODE>
__global__ __launch_bounds__(256) void k_grm_finish(const double *__restrict__ S, const uint32_t *__restrict__ n, size_t ld, uint64_t i0, uint64_t ni,
                                                     uint64_t nj, int divisor, double P, double *__restrict__ out, uint32_t *__restrict__ out_n,
                                                     const uint8_t *__restrict__ keep, double thr, uint64_t cap,
                                                     unsigned long long *__restrict__ count, uint32_t *__restrict__ out_i,
                                                     uint32_t *__restrict__ out_j)
{
   const uint64_t b = (uint64_t)blockIdx.x * 256 + threadIdx.x, a = blockIdx.y;
   if (b >= nj || a >= ni) return;
   const uint64_t i = i0 + a;
   if (MODE == GRM_TRI && b > i) return;
   if (MODE == GRM_PAIRS && (b >= i || (keep && (!keep[i] || !keep[b])))) return;
   const size_t at = (size_t)a * ld + b;
   const uint32_t cnt = n ? n[at] : 0u;
   const double v = grm_value(S[at], divisor, cnt, P);
   if (MODE == GRM_RECT) {
      out[at] = v;
   } else if (MODE == GRM_TRI) {
      const size_t o = (size_t)(i * (i + 1) / 2 - i0 * (i0 + 1) / 2 + b);
      out[o] = v;
      if (out_n) out_n[o] = cnt;
   } else if (v > thr) {
      const unsigned long long slot = atomicAdd(count, 1ull);
      if (slot < cap) {
         out_i[slot] = (uint32_t)b;
         out_j[slot] = (uint32_t)i;
         out[slot] = v;
         if (out_n) out_n[slot] = cnt;
      }
   }
}

// what every entry point refuses (before any device work): the refusals of king.hip
void grm_refuse(const fpca_ctx *c, const char *fn)
{
   if (!c) throw Error(FPCA_EINVAL, std::string("bad argument to ") + fn + " (NULL context)");
   if (c->dense)
      throw Error(FPCA_EINVAL, std::string(fn) + ": this context holds a dense matrix; the relationship matrix is computed from the packed genotypes "
                                                 "(fpca_create, fpca_create_from_bed, synthetic)");
   if (c->masked())
      throw Error(FPCA_EINVAL, std::string(fn) + ": a sample mask is set (fpca_set_sample_mask); clear it (the pair calls take a mask as `keep`)");
   if (c->multi() || (c->rank_known && c->nranks > 1))
      throw Error(FPCA_EINVAL, std::string(fn) + ": this context is one shard of several (a communicator, an all-reduce hook or fpca_set_rank with "
                                                 "more than one rank); the relationship matrix sums over all SNPs -- compute it on a single context");
   if (c->P_g > GRM_MAX_P)
      throw Error(FPCA_EINVAL, std::string(fn) + ": " + std::to_string(c->P_g) + " SNPs; above 2^28 = 268,435,456 the shared-call counts no longer fit 32 bits");
   if (c->N > 0xFFFFFFFFull) throw Error(FPCA_EINVAL, std::string(fn) + ": this context has " + std::to_string(c->N) + " samples; at most 2^32 - 1");
}

void grm_check_divisor(const char *fn, int divisor)
{
   if (divisor != FPCA_GRM_DIV_SHARED && divisor != FPCA_GRM_DIV_P && divisor != FPCA_GRM_DIV_NONE)
      throw Error(FPCA_EINVAL, std::string(fn) + ": divisor " + std::to_string(divisor) +
                                   " is none of FPCA_GRM_DIV_SHARED (0), FPCA_GRM_DIV_P (1), FPCA_GRM_DIV_NONE (2)");
}

bool grm_force_general()
{
   const char *v = FPCA_TEST_ENV("FPCA_GRM_FORCE_GENERAL");
   return v && *v && *v != '0';
}

// device buffers of one call
struct GrmBufs {
   DevMem<uint8_t> d_smp, d_dead, d_keep; // the sample-major copy [N_pad][pitch]; the non-live mask [pitch]; keep [N]
   size_t pitch = 0;
   DevMem<uint32_t> d_tot, d_live; // per-sample totals; the live-SNP count
   // the slab: S and n [rows][ld], the output (the rectangle / packed rows) and its counts
   DevMem<double> d_S, d_out;
   DevMem<uint32_t> d_n, d_out_n;
   size_t ld = 0;
   // the pair list
   DevMem<uint32_t> d_i, d_j, d_pn;
   DevMem<double> d_g;
   DevMem<unsigned long long> d_count;
   bool counts = false; // k_grm_shared runs
   void alloc_pairs(size_t slots, bool with_n, const char *fn)
   {
      d_i = DevMem<uint32_t>(slots, fn, "the pair list (i)");
      d_j = DevMem<uint32_t>(slots, fn, "the pair list (j)");
      d_g = DevMem<double>(slots, fn, "the pair list (g)");
      if (with_n) d_pn = DevMem<uint32_t>(slots, fn, "the pair list (shared)");
      d_count = DevMem<unsigned long long>(1, fn, "the pair counter");
   }
};

// the sample-major operand with the non-live SNPs read as missing, its per-sample totals and the live count, on the context's stream
void grm_make_operand(fpca_ctx *c, GrmBufs &s, const char *fn)
{
   ensure_stats(c);
   s.pitch = (size_t)round_up(c->P_pad / 4, 128);
   const size_t need = (size_t)c->N_pad * s.pitch;
   char detail[96];
   std::snprintf(detail, sizeof(detail), "%llu samples x %llu bytes", (unsigned long long)c->N_pad, (unsigned long long)s.pitch);
   s.d_smp = DevMem<uint8_t>(need, fn, "sample-major copy", 0, detail, c->device);
   HIP_CHECK(hipMemsetAsync(s.d_smp.p, PAD_BYTE, need, c->stream));
   kern::transpose_packed(c->d_packed, c->pitch, c->N_pad, c->P_pad, s.d_smp.p, s.pitch, c->stream, false);
   s.d_dead = DevMem<uint8_t>(s.pitch, fn, "the non-live SNP mask");
   s.d_live = DevMem<uint32_t>(1, fn, "the live SNP count");
   HIP_CHECK(hipMemsetAsync(s.d_live.p, 0, sizeof(uint32_t), c->stream));
   hipLaunchKernelGGL(k_grm_live, dim3((unsigned)((s.pitch + 255) / 256)), dim3(256), 0, c->stream, c->d_lut, c->P_g, s.pitch, s.d_dead.p, s.d_live.p);
   launch_check();
   const uint64_t vecs = c->N * (s.pitch / 16);
   hipLaunchKernelGGL(k_grm_kill, dim3((unsigned)((vecs + 255) / 256)), dim3(256), 0, c->stream, s.d_smp.p, s.pitch, c->N, s.d_dead.p);
   launch_check();
   s.d_tot = DevMem<uint32_t>(c->N * 4, fn, "the per-sample totals");
   kern::ld_totals(s.d_smp.p, s.pitch, c->N, s.d_tot.p, c->stream);
}

// rows of a slab whose cells are `cols` wide: S and n within GRM_SLAB_BYTES, the tile pairs within one launch; a multiple of the tile, at least one
uint64_t grm_slab_rows(uint64_t cols)
{
   uint64_t forced = 0;
   if (const char *v = FPCA_TEST_ENV("FPCA_GRM_SLAB_ROWS"))
      if (std::atoll(v) > 0) forced = ((uint64_t)std::atoll(v) + GRM_TILE - 1) / GRM_TILE * GRM_TILE;
   if (forced) return forced;
   const uint64_t by_mem = GRM_SLAB_BYTES / (cols * (sizeof(double) + sizeof(uint32_t))) / GRM_TILE;
   const uint64_t by_launch = GRM_LAUNCH_PAIRS / ((cols + GRM_TILE - 1) / GRM_TILE);
   return std::min<uint64_t>(std::max<uint64_t>(std::min(by_mem, by_launch), 1), 512) * GRM_TILE; // (a row is one grid.y of k_grm_finish)
}

// the slab scratch for slabs of up to `rows` rows of `cols` cells; packed: the output holds packed triangle rows, else a rectangle
void grm_alloc_slab(const fpca_ctx *c, GrmBufs &s, uint64_t rows, uint64_t cols, int mode, bool out_counts, const char *fn)
{
   s.ld = (size_t)cols;
   const size_t cells = (size_t)rows * cols;
   char detail[128];
   std::snprintf(detail, sizeof(detail), "a slab of %llu rows x %llu samples", (unsigned long long)rows, (unsigned long long)cols);
   s.d_S = DevMem<double>(cells, fn, "slab scratch (sums)", 0, detail, c->device);
   if (s.counts) s.d_n = DevMem<uint32_t>(cells, fn, "slab scratch (shared calls)", 0, detail, c->device);
   if (mode == GRM_PAIRS) return;
   s.d_out = DevMem<double>(cells, fn, "slab scratch (output)", 0, detail, c->device);
   if (mode == GRM_TRI && out_counts) s.d_out_n = DevMem<uint32_t>(cells, fn, "slab scratch (output counts)", 0, detail, c->device);
}

// S (and n) of the cells [i0, iend) x [j0, jend) into the slab scratch
void grm_products(const fpca_ctx *c, const GrmBufs &s, bool tri, uint64_t i0, uint64_t iend, uint64_t j0, uint64_t jend, bool dot = true,
                  bool shared = true)
{
   const uint64_t nti = (iend - i0 + GRM_TILE - 1) / GRM_TILE, ntj = (jend - j0 + GRM_TILE - 1) / GRM_TILE, wgs = nti * ntj;
   if (!wgs) return;
   if (wgs > 0x7FFFFFFFull || ntj > 0xFFFFFFFFull)
      throw Error(FPCA_EINVAL, "relationship matrix: " + std::to_string(wgs) + " tile pairs exceed one launch");
   const dim3 grid((unsigned)wgs), block(256);
   if (dot) {
      if (tri)
         hipLaunchKernelGGL(k_grm_dot<true>, grid, block, 0, c->stream, s.d_smp.p, s.pitch, c->d_lut, c->P_g, c->N, i0, iend, j0, jend, (uint32_t)ntj,
                            s.d_S.p, s.ld);
      else
         hipLaunchKernelGGL(k_grm_dot<false>, grid, block, 0, c->stream, s.d_smp.p, s.pitch, c->d_lut, c->P_g, c->N, i0, iend, j0, jend, (uint32_t)ntj,
                            s.d_S.p, s.ld);
      launch_check();
   }
   if (shared && s.counts) {
      if (tri)
         hipLaunchKernelGGL(k_grm_shared<true>, grid, block, 0, c->stream, s.d_smp.p, s.pitch, s.d_tot.p, s.d_live.p, c->N, i0, iend, j0, jend,
                            (uint32_t)ntj, (int)grm_force_general(), s.d_n.p, s.ld);
      else
         hipLaunchKernelGGL(k_grm_shared<false>, grid, block, 0, c->stream, s.d_smp.p, s.pitch, s.d_tot.p, s.d_live.p, c->N, i0, iend, j0, jend,
                            (uint32_t)ntj, (int)grm_force_general(), s.d_n.p, s.ld);
      launch_check();
   }
}

void grm_finish(int mode, const fpca_ctx *c, const GrmBufs &s, uint64_t i0, uint64_t ni, uint64_t nj, int divisor, double thr, uint64_t cap)
{
   const dim3 grid((unsigned)((nj + 255) / 256), (unsigned)ni), block(256);
   const double P = (double)c->P_g;
#define GRM_FINISH(M)                                                                                                                          \
   hipLaunchKernelGGL(k_grm_finish<M>, grid, block, 0, c->stream, s.d_S.p, s.d_n.p, s.ld, i0, ni, nj, divisor, P, M == GRM_PAIRS ? s.d_g.p : s.d_out.p, \
                      M == GRM_PAIRS ? s.d_pn.p : s.d_out_n.p, s.d_keep.p, thr, cap, s.d_count.p, s.d_i.p, s.d_j.p)
   if (mode == GRM_RECT)
      GRM_FINISH(GRM_RECT);
   else if (mode == GRM_TRI)
      GRM_FINISH(GRM_TRI);
   else
      GRM_FINISH(GRM_PAIRS);
#undef GRM_FINISH
   launch_check();
}

// rows of the triangle's slabs: slab [a, b) has the columns [0, b)
uint64_t grm_tri_rows(uint64_t N) { return std::min<uint64_t>(grm_slab_rows(N), (N + GRM_TILE - 1) / GRM_TILE * GRM_TILE); }

struct GrmPair {
   uint32_t i, j, n;
   double g;
};

// the pair pass: every pair i < j of kept samples with G > thr, sorted by (i, j), when no more than `cap` qualify; returns how many do
uint64_t grm_pair_pass(fpca_ctx *c, const char *fn, const uint8_t *keep, double thr, int divisor, bool want_n, uint64_t cap, std::vector<GrmPair> &out)
{
   const uint64_t N = c->N;
   cap = std::min<uint64_t>(cap, N * (N - 1) / 2);
   HIP_CHECK(hipSetDevice(c->device));
   GrmBufs s;
   s.counts = divisor == FPCA_GRM_DIV_SHARED || want_n;
   grm_make_operand(c, s, fn);
   if (keep) {
      s.d_keep = DevMem<uint8_t>(N, fn, "the sample mask");
      HIP_CHECK(hipMemcpyAsync(s.d_keep.p, keep, N, hipMemcpyHostToDevice, c->stream));
   }
   s.alloc_pairs((size_t)std::max<uint64_t>(cap, 1), want_n, fn);
   HIP_CHECK(hipMemsetAsync(s.d_count.p, 0, sizeof(unsigned long long), c->stream));
   const uint64_t rows = grm_tri_rows(N);
   grm_alloc_slab(c, s, rows, N, GRM_PAIRS, false, fn);
   for (uint64_t a = 0; a < N; a += rows) {
      const uint64_t b = std::min(a + rows, N);
      grm_products(c, s, true, a, b, 0, b);
      grm_finish(GRM_PAIRS, c, s, a, b - a, b, divisor, thr, cap);
   }
   unsigned long long found = 0;
   HIP_CHECK(hipMemcpyAsync(&found, s.d_count.p, sizeof(found), hipMemcpyDeviceToHost, c->stream));
   HIP_CHECK(hipStreamSynchronize(c->stream));
   out.clear();
   if (found > cap || found == 0) return found;
   std::vector<uint32_t> hi(found), hj(found), hn(want_n ? found : 0);
   std::vector<double> hg(found);
   HIP_CHECK(hipMemcpy(hi.data(), s.d_i.p, found * sizeof(uint32_t), hipMemcpyDeviceToHost));
   HIP_CHECK(hipMemcpy(hj.data(), s.d_j.p, found * sizeof(uint32_t), hipMemcpyDeviceToHost));
   HIP_CHECK(hipMemcpy(hg.data(), s.d_g.p, found * sizeof(double), hipMemcpyDeviceToHost));
   if (want_n) HIP_CHECK(hipMemcpy(hn.data(), s.d_pn.p, found * sizeof(uint32_t), hipMemcpyDeviceToHost));
   out.resize(found);
   for (uint64_t k = 0; k < found; k++) out[k] = {hi[k], hj[k], want_n ? hn[k] : 0u, hg[k]};
   std::sort(out.begin(), out.end(), [](const GrmPair &a, const GrmPair &b) { return a.i != b.i ? a.i < b.i : a.j < b.j; });
   return found;
}

} // namespace

extern "C" int fpca_grm_block(fpca_ctx *ctx, uint64_t i0, uint64_t ni, uint64_t j0, uint64_t nj, int divisor, double *grm, uint32_t *shared)
{
   return guarded([&] {
      const char *fn = "fpca_grm_block";
      grm_refuse(ctx, fn);
      if (!grm) throw Error(FPCA_EINVAL, "bad argument to fpca_grm_block (grm is NULL)");
      grm_check_divisor(fn, divisor);
      const uint64_t N = ctx->N;
      if (ni == 0 || nj == 0 || i0 >= N || ni > N - i0 || j0 >= N || nj > N - j0)
         throw Error(FPCA_EINVAL, "fpca_grm_block: samples [" + std::to_string(i0) + ", " + std::to_string(i0) + " + " + std::to_string(ni) + ") x [" +
                                      std::to_string(j0) + ", " + std::to_string(j0) + " + " + std::to_string(nj) +
                                      ") are not a non-empty rectangle of this context's " + std::to_string(N) + " samples");
      if (ni > GRM_BLOCK_LIMIT / sizeof(double) / nj)
         throw Error(FPCA_EINVAL, "fpca_grm_block: a block of " + std::to_string(ni) + " x " + std::to_string(nj) + " doubles is over the limit of " +
                                      std::to_string(GRM_BLOCK_LIMIT) + " bytes; call it block by block");
      HIP_CHECK(hipSetDevice(ctx->device));
      GrmBufs s;
      s.counts = divisor == FPCA_GRM_DIV_SHARED || shared;
      grm_make_operand(ctx, s, fn);
      const uint64_t rows = std::min<uint64_t>(grm_slab_rows(nj), (ni + GRM_TILE - 1) / GRM_TILE * GRM_TILE);
      grm_alloc_slab(ctx, s, rows, nj, GRM_RECT, false, fn);
      for (uint64_t a = i0; a < i0 + ni; a += rows) {
         const uint64_t b = std::min(a + rows, i0 + ni);
         const size_t cells = (size_t)(b - a) * nj, at = (size_t)(a - i0) * nj;
         grm_products(ctx, s, false, a, b, j0, j0 + nj);
         grm_finish(GRM_RECT, ctx, s, a, b - a, nj, divisor, 0.0, 0);
         HIP_CHECK(hipMemcpyAsync(grm + at, s.d_out.p, cells * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
         if (shared) HIP_CHECK(hipMemcpyAsync(shared + at, s.d_n.p, cells * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
      }
      HIP_CHECK(hipStreamSynchronize(ctx->stream));
   });
}

extern "C" int fpca_grm_tri(fpca_ctx *ctx, int divisor, double *grm, uint32_t *shared)
{
   return guarded([&] {
      const char *fn = "fpca_grm_tri";
      grm_refuse(ctx, fn);
      if (!grm) throw Error(FPCA_EINVAL, "bad argument to fpca_grm_tri (grm is NULL)");
      grm_check_divisor(fn, divisor);
      const uint64_t N = ctx->N;
      HIP_CHECK(hipSetDevice(ctx->device));
      GrmBufs s;
      s.counts = divisor == FPCA_GRM_DIV_SHARED || shared;
      grm_make_operand(ctx, s, fn);
      const uint64_t rows = grm_tri_rows(N);
      grm_alloc_slab(ctx, s, rows, N, GRM_TRI, shared != nullptr, fn);
      for (uint64_t a = 0; a < N; a += rows) {
         const uint64_t b = std::min(a + rows, N);
         const size_t at = (size_t)(a * (a + 1) / 2), cells = (size_t)(b * (b + 1) / 2) - at; // the packed rows a .. b - 1
         grm_products(ctx, s, true, a, b, 0, b);
         grm_finish(GRM_TRI, ctx, s, a, b - a, b, divisor, 0.0, 0);
         // the slab goes to the host as it finishes; the next one's kernels queue behind the copy
         HIP_CHECK(hipMemcpyAsync(grm + at, s.d_out.p, cells * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
         if (shared) HIP_CHECK(hipMemcpyAsync(shared + at, s.d_out_n.p, cells * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
      }
      HIP_CHECK(hipStreamSynchronize(ctx->stream));
   });
}

extern "C" int fpca_grm_pairs(fpca_ctx *ctx, const uint8_t *keep, double thr, int divisor, uint64_t max_pairs, uint32_t *i, uint32_t *j, double *g,
                              uint32_t *shared, uint64_t *n_pairs)
{
   return guarded([&] {
      grm_refuse(ctx, "fpca_grm_pairs");
      if (!n_pairs || (max_pairs && (!i || !j || !g))) throw Error(FPCA_EINVAL, "bad argument to fpca_grm_pairs (a NULL output)");
      if (std::isnan(thr)) throw Error(FPCA_EINVAL, "fpca_grm_pairs: the threshold is NaN");
      grm_check_divisor("fpca_grm_pairs", divisor);
      std::vector<GrmPair> pairs;
      const uint64_t found = grm_pair_pass(ctx, "fpca_grm_pairs", keep, thr, divisor, shared != nullptr, max_pairs, pairs);
      *n_pairs = found;
      if (found > max_pairs)
         throw Error(FPCA_ENOMEM, "fpca_grm_pairs: " + std::to_string(found) + " pairs are above the threshold, the arrays hold " +
                                      std::to_string(max_pairs) + "; call again with room for " + std::to_string(found));
      for (uint64_t k = 0; k < found; k++) {
         i[k] = pairs[k].i;
         j[k] = pairs[k].j;
         g[k] = pairs[k].g;
         if (shared) shared[k] = pairs[k].n;
      }
   });
}

extern "C" int fpca_grm_cutoff(fpca_ctx *ctx, double thr, int divisor, uint8_t *keep, uint64_t *n_kept)
{
   return guarded([&] {
      grm_refuse(ctx, "fpca_grm_cutoff");
      if (!keep) throw Error(FPCA_EINVAL, "bad argument to fpca_grm_cutoff (keep is NULL)");
      if (std::isnan(thr)) throw Error(FPCA_EINVAL, "fpca_grm_cutoff: the threshold is NaN");
      grm_check_divisor("fpca_grm_cutoff", divisor);
      uint64_t cap = GRM_CUTOFF_CAP;
      if (const char *v = FPCA_TEST_ENV("FPCA_GRM_MAX_PAIRS"))
         if (std::atoll(v) > 0) cap = (uint64_t)std::atoll(v);
      std::vector<GrmPair> pairs;
      const uint64_t found = grm_pair_pass(ctx, "fpca_grm_cutoff", keep, thr, divisor, false, cap, pairs);
      if (found > cap)
         throw Error(FPCA_ENOMEM, "fpca_grm_cutoff: " + std::to_string(found) + " pairs are above the threshold, the call keeps room for " +
                                      std::to_string(cap) + "; raise the threshold or thin the samples first (fpca_grm_pairs lists them)");
      std::vector<uint32_t> pi(found), pj(found);
      for (uint64_t k = 0; k < found; k++) {
         pi[k] = pairs[k].i;
         pj[k] = pairs[k].j;
      }
      const uint64_t kept = king_cutoff_rule(pi.data(), pj.data(), found, ctx->N, keep);
      if (n_kept) *n_kept = kept;
   });
}

extern "C" int fpca_bench_grm(fpca_ctx *ctx, int reps, double *ms, double *flops)
{
   return guarded([&] {
      const char *fn = "fpca_bench_grm";
      grm_refuse(ctx, fn);
      if (!ms || reps < 1) throw Error(FPCA_EINVAL, "bad argument to fpca_bench_grm");
      HIP_CHECK(hipSetDevice(ctx->device));
      const uint64_t N = ctx->N;
      GrmBufs s;
      s.counts = true;
      grm_make_operand(ctx, s, fn);
      const uint64_t rows = grm_tri_rows(N);
      grm_alloc_slab(ctx, s, rows, N, GRM_PAIRS, false, fn);
      // the FP64 Gram kernel alone over the whole triangle, slab by slab as fpca_grm_tri launches it (test build, FPCA_GRM_BENCH_SHARED=1: the
      // count kernel alone instead)
      const char *v = FPCA_TEST_ENV("FPCA_GRM_BENCH_SHARED");
      const bool count_kernel = v && *v && *v != '0';
      DevEvent e0(fn), e1(fn);
      for (int r = -1; r < reps; r++) { // one untimed pass first
         HIP_CHECK(hipEventRecord(e0, ctx->stream));
         for (uint64_t a = 0; a < N; a += rows) grm_products(ctx, s, true, a, std::min(a + rows, N), 0, std::min(a + rows, N), !count_kernel, count_kernel);
         HIP_CHECK(hipEventRecord(e1, ctx->stream));
         HIP_CHECK(hipEventSynchronize(e1));
         if (r >= 0) ms[r] = elapsed_ms(e0, e1);
      }
      if (flops) { // the 32 x 32 wave blocks on or below the diagonal, each 2 x 32 x 32 x (4 pitch) flops
         const double nb = (double)((N + 31) / 32), blocks = nb * (nb + 1.0) / 2.0;
         *flops = blocks * 2.0 * 32.0 * 32.0 * 4.0 * (double)s.pitch;
      }
   });
}
