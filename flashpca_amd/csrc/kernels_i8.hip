// kernels_i8.hip -- exact-integer flavour of the two genotype GEMMs (FPCA_ACCUM_I8(S)).
//
// A standardised genotype is x_ij = m_ij (g_ij - mu_j) / sigma_j with g in {0,1,2} the dosage and m in {0,1} the
// "not missing" flag, so
//     T = X' B = diag(1/sigma) [ (G.M)' B  -  diag(mu) M' B ]           (K2)
//     Y = X T  = (G.M) (T / sigma)  -  M (mu T / sigma)                  (K3)
// where G.M and M are tiny integers.  The fp64 operand (B, resp. T/sigma and mu T/sigma) is rounded per column to a
// (8S-2)-bit fixed-point number sharing one power-of-two scale (m = rint(v 2^(8S-2-e)), 2^e > max|column|) and cut into
// its S two's-complement bytes (m = sum_i d_i 256^i, d_i in [-128, 127], the top one within +-65): full 8-bit digits,
// so S = 7 keeps 54 bits below the column maximum.  The products run on v_mfma_i32_32x32x32_i8 with EXACT int32
// accumulation (|sum| <= 256 K).  The only rounding of the whole product is the 2^-(8S-2) rounding of the fp64 operand
// and the fp64 recombination of the S exact slice sums (once per split-K part) -- nothing accumulates along K -- so
// S = 7 is fp64-equivalent while the int8 MFMA issues 64x the multiply-adds per cycle of the fp64 one for 14x as many.
//
// MFMA operand maps (32x32x32 i8): lane l holds 16 int8 of A row i = l&31 and of B column j = l&31 for the K-half
// l>>5; A and B use the same (half, byte) -> k assignment, so the dot products do not depend on it.  C/D register r of
// lane l is D[row = (r&3) + 8 (r>>2) + 4 (l>>5)][col = l&31].
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <type_traits>
#include <utility>

#include "common.hpp"
#include "dev_scratch.hpp"
#include "kernels.hpp"
#include "launch_check.hpp"

namespace fpca {
namespace kern {

typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v16i __attribute__((ext_vector_type(16)));
typedef double d2 __attribute__((ext_vector_type(2)));
typedef uint32_t u4 __attribute__((ext_vector_type(4)));
typedef uint32_t u2 __attribute__((ext_vector_type(2)));

// ------------------------------------------------------------------------------------------------
// slicing of an fp64 operand V[rows_pad][b] (row-major, rows = samples for K2, SNPs for K3) into
// Q[S*b][rows_pad] int8 (slice-column sc = s*b + c, contiguous along the rows = the GEMM's K dimension).
// Inside every aligned group of 16 rows the bytes are stored in the order the decoded genotype operand uses:
// position 4q + t holds row q + 4t (see decode in k_gemm_i8).

// One pass over V can serve two operands that differ only by a per-row factor (K3: T/sd and mean T/sd).
//
// Column maxima travel as the bit patterns of non-negative doubles (they order like integers, so an integer
// atomicMax is exact); the caller zeroes them -- and the column sums -- once per apply.

// Both kinds of accumulator are sharded I8_SHARDS ways by block index: same-address atomics serialise in L2 (~20 ns
// each), and with hundreds of blocks that was longer than the kernels' useful work.  Consumers fold the shards.
// maxbits: [I8_SHARDS][64], colsum: [I8_SHARDS][I8_CS_STRIDE]

// block-level max over the 256/b row slots of each column, then one atomic per column
__device__ __forceinline__ void colmax_commit(double m, int b, double *smax /* [256] */, unsigned long long *bits)
{
   __syncthreads();
   smax[threadIdx.x] = m;
   __syncthreads();
   if ((int)threadIdx.x < b) {
      for (int k = 1; k < 256 / b; k++) m = fmax(m, smax[k * b + threadIdx.x]);
      atomicMax(&bits[(blockIdx.x % I8_SHARDS) * 64 + threadIdx.x], (unsigned long long)__double_as_longlong(m));
   }
}

__device__ __forceinline__ unsigned long long maxbits_fold(const unsigned long long *bits, int c)
{
   unsigned long long m = 0;
#pragma unroll
   for (int k = 0; k < I8_SHARDS; k++) m = bits[k * 64 + c] > m ? bits[k * 64 + c] : m;
   return m;
}
__device__ __forceinline__ long long colsum_fold(const long long *cs, int t)
{
   long long a = 0;
#pragma unroll
   for (int k = 0; k < I8_SHARDS; k++) a += cs[k * I8_CS_STRIDE + t];
   return a;
}

// per-column max |v * rowscale| for one or two row scalings (standalone pass; the hot path gets K3's maxima from the
// K2 combine instead)
template <int NOPS>
__global__ __launch_bounds__(256) void k_colmax(const double *__restrict__ V, uint64_t rows, int b, const double *__restrict__ rs0,
                                                unsigned long long *__restrict__ bits0, const double *__restrict__ rs1,
                                                unsigned long long *__restrict__ bits1)
{
   __shared__ double smax[256];
   const int c = threadIdx.x % b;
   const int r_in = threadIdx.x / b, r_step = 256 / b;
   double m0[4] = {0, 0, 0, 0}, m1[4] = {0, 0, 0, 0}; // 4 independent chains: 4 loads in flight per thread
   if (r_in < r_step) {
      const uint64_t stride = (uint64_t)gridDim.x * r_step;
      for (uint64_t r = (uint64_t)blockIdx.x * r_step + r_in; r < rows; r += 4 * stride) {
#pragma unroll
         for (int u = 0; u < 4; u++) {
            const uint64_t rr = r + u * stride;
            if (rr < rows) {
               const double v = V[rr * b + c];
               const double a = fabs(rs0 ? v * rs0[rr] : v);
               if (a > m0[u]) m0[u] = a; // NaN never wins: a NaN operand would poison the fp64 path as well
               if (NOPS == 2) {
                  const double a1 = fabs(v * rs1[rr]);
                  if (a1 > m1[u]) m1[u] = a1;
               }
            }
         }
      }
   }
   colmax_commit(fmax(fmax(m0[0], m0[1]), fmax(m0[2], m0[3])), b, smax, bits0);
   if (NOPS == 2) colmax_commit(fmax(fmax(m1[0], m1[1]), fmax(m1[2], m1[3])), b, smax, bits1);
}

// scale of column c: 2^e > max|column| (e from frexp; zero column -> e = 0)
__device__ __forceinline__ int slice_exponent(unsigned long long bits)
{
   const double m = __longlong_as_double((long long)bits);
   int e = 0;
   if (m > 0.0 && isfinite(m)) (void)frexp(m, &e); // m = f 2^e, f in [0.5, 1)  =>  m < 2^e
   return e;
}

// one thread = one 16-row group of one column: 16 strided fp64 in, one 16-byte store per slice and operand out; block 0
// also writes the weights colw[s*b + c] = 2^(e_c - (8S-2)) 256^(S-1-s) (slice 0 = top byte; 0 for the padding
// slice-columns); optionally the exact
// integer column sums of every slice (for  M'Q = 1'Q - E'Q, see k_gemm_i8) -- block-reduced, one atomic per
// slice-column per block
template <int NOPS>
__global__ __launch_bounds__(256) void k_slice(const double *__restrict__ V, uint64_t rows_pad, uint64_t rows, int b, int S, int nsc_pad,
                                               SliceOp o0, SliceOp o1)
{
   __shared__ int ssum[NOPS][9][256];
   const uint64_t groups = rows_pad / 16;
   const int c = threadIdx.x % b, gl = threadIdx.x / b, gpb = 256 / b; // column, local group, groups per block
   const SliceOp *ops[2] = {&o0, &o1};
   const int F = 8 * S - 2; // fractional bits below 2^e; |m| < 2^F <= 2^62
   int sh[NOPS];
#pragma unroll
   for (int o = 0; o < NOPS; o++) {
      const int e = slice_exponent(maxbits_fold(ops[o]->maxbits, c));
      sh[o] = F - e;
      if (blockIdx.x == 0) {
         if (gl == 0)
            for (int s = 0; s < S; s++) ops[o]->colw[s * b + c] = ldexp(1.0, e - F + 8 * (S - 1 - s));
         for (int t = S * b + threadIdx.x; t < nsc_pad; t += 256) ops[o]->colw[t] = 0.0;
      }
   }
   for (uint64_t g0 = (uint64_t)blockIdx.x * gpb; g0 < groups; g0 += (uint64_t)gridDim.x * gpb) {
      const uint64_t g = g0 + gl;
      const bool act = gl < gpb && g < groups;
      const uint64_t r0 = g * 16;
      double v[16];
#pragma unroll
      for (int j = 0; j < 16; j++) {
         const uint64_t r = r0 + j;
         v[j] = (act && r < rows) ? V[r * b + c] : 0.0;
      }
#pragma unroll
      for (int o = 0; o < NOPS; o++) {
         long long m[16];
#pragma unroll
         for (int j = 0; j < 16; j++) {
            const uint64_t r = r0 + j;
            double x = v[j];
            if (ops[o]->rowscale && act && r < rows) x *= ops[o]->rowscale[r];
            m[j] = __double2ll_rn(ldexp(x, sh[o])); // power-of-two scaling is exact; |m| < 2^F
            if (ops[o]->copy64 && act && r < rows) ops[o]->copy64[r * b + c] = x;
            if (ops[o]->copy32 && act && r < rows) ops[o]->copy32[r * b + c] = (float)ldexp(x, sh[o] - F + 1); // |.| < 2: any column fits fp32
         }
         for (int s = S - 1; s >= 0; s--) { // bytes from the low end, carries into the next one
            u4 word = {0u, 0u, 0u, 0u};
            int tot = 0;
#pragma unroll
            for (int j = 0; j < 16; j++) {
               const int d = (int)(signed char)(m[j] & 0xFF);
               m[j] = (m[j] - d) >> 8;
               tot += d;
               word[j & 3] |= ((uint32_t)d & 0xFFu) << (8 * (j >> 2)); // position 4 (j&3) + (j>>2)
            }
            if (act) *reinterpret_cast<u4 *>(ops[o]->Q + ((uint64_t)(s * b + c)) * rows_pad + r0) = word;
            ssum[o][s][threadIdx.x] = tot;
         }
      }
      if (o0.colsum || (NOPS == 2 && o1.colsum)) {
         __syncthreads();
#pragma unroll
         for (int o = 0; o < NOPS; o++)
            if (ops[o]->colsum)
               for (int t = threadIdx.x; t < S * b; t += 256) {
                  const int s = t / b, cc = t % b;
                  long long a = 0;
                  for (int k = 0; k < gpb; k++) a += ssum[o][s][k * b + cc];
                  if (a)
                     atomicAdd(reinterpret_cast<unsigned long long *>(&ops[o]->colsum[(blockIdx.x % I8_SHARDS) * I8_CS_STRIDE + t]),
                               (unsigned long long)a);
               }
         __syncthreads();
      }
   }
}

int gemm_i8_nsc_pad(int S, int b);

void i8_colmax(const double *V, uint64_t rows, int b, int nops, const SliceOp *ops, hipStream_t stream)
{
   const unsigned blocks = (unsigned)std::min<uint64_t>(1024, rows * b / 1024 + 1);
   if (nops == 2)
      hipLaunchKernelGGL(k_colmax<2>, dim3(blocks), dim3(256), 0, stream, V, rows, b, ops[0].rowscale, ops[0].maxbits, ops[1].rowscale,
                         ops[1].maxbits);
   else
      hipLaunchKernelGGL(k_colmax<1>, dim3(blocks), dim3(256), 0, stream, V, rows, b, ops[0].rowscale, ops[0].maxbits, nullptr, nullptr);
   launch_check();
}

void i8_slice(const double *V, uint64_t rows_pad, uint64_t rows, int b, int S, int nops, const SliceOp *ops, hipStream_t stream)
{
   if (S > 8 || b > 64 || nops < 1 || nops > 2) throw Error(-1, "i8_slice: S <= 8, b <= 64, 1 or 2 operands");
   const unsigned blocks = (unsigned)std::min<uint64_t>(4096, (rows_pad / 16 + (256 / b) - 1) / (256 / b));
   const int nsc = gemm_i8_nsc_pad(S, b);
   if (nops == 2)
      hipLaunchKernelGGL(k_slice<2>, dim3(blocks), dim3(256), 0, stream, V, rows_pad, rows, b, S, nsc, ops[0], ops[1]);
   else
      hipLaunchKernelGGL(k_slice<1>, dim3(blocks), dim3(256), 0, stream, V, rows_pad, rows, b, S, nsc, ops[0], ops[0]);
   launch_check();
}

// ------------------------------------------------------------------------------------------------
// Row-sharded operand exchange (round 6; operator.hip apply_sharded): every rank slices ITS rows of the block and the ranks
// all-gather the SLICES -- S bytes per entry instead of the 8 of the fp64 block -- in a ROW-MAJOR layout Qrm[row][s*b + c]
// (a rank's rows of a chunk are one contiguous piece, so the gathered buffer is simply [all rows][S*b] in global row order).
//   k_maxbits_fold / k_maxbits_set   the column maxima: shards folded for the exchange / the maximum over all ranks' answers put back
//   k_slice_rows                     V[rows][b] fp64 -> Qrm[rows][S*b] with the GLOBAL column scales; thread = (row, 16 columns)
//   k_unpack_slices                  Qrm[rows_pad][S*b] -> Q[s*b + c][rows_pad] in the 16-row-group byte order of k_slice + the exact
//                                    column sums of every slice; thread = (16 rows, slice, 16 columns)
//   k_dequant_rows                   Qrm -> the scaled operand itself for the sparse gathers of the missing-call route: fp32 rows
//                                    m 2^(1-F) (<= 4 slices) or fp64 rows m 2^(e-F); m = the (8S-2)-bit integer the slices spell --
//                                    exactly the operand the GEMM multiplies
__global__ void k_maxbits_fold(const unsigned long long *__restrict__ bits, double *__restrict__ out)
{
   if (threadIdx.x < 64) out[threadIdx.x] = __longlong_as_double((long long)maxbits_fold(bits, threadIdx.x));
}
__global__ void k_maxbits_set(const double *__restrict__ all, int G, unsigned long long *__restrict__ bits)
{
   if (threadIdx.x < 64) {
      double m = 0.0;
      for (int g = 0; g < G; g++) m = fmax(m, all[g * 64 + threadIdx.x]);
      bits[threadIdx.x] = (unsigned long long)__double_as_longlong(m);
      for (int k = 1; k < I8_SHARDS; k++) bits[k * 64 + threadIdx.x] = 0ull;
   }
}

__global__ __launch_bounds__(256) void k_slice_rows(const double *__restrict__ V, uint64_t rows, int b, int S, int nsc_pad,
                                                    const unsigned long long *__restrict__ maxbits, int8_t *__restrict__ Qrm,
                                                    double *__restrict__ colw)
{
   __shared__ int sh_e[64];
   const int F = 8 * S - 2;
   if ((int)threadIdx.x < b) {
      const int e = slice_exponent(maxbits_fold(maxbits, threadIdx.x));
      sh_e[threadIdx.x] = e;
      if (blockIdx.x == 0)
         for (int s = 0; s < S; s++) colw[s * b + threadIdx.x] = ldexp(1.0, e - F + 8 * (S - 1 - s));
   }
   if (blockIdx.x == 0)
      for (int t = S * b + threadIdx.x; t < nsc_pad; t += 256) colw[t] = 0.0;
   __syncthreads();
   const int gpr = b / 16; // 16-column groups per row
   const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x, row = t / gpr;
   const int g = (int)(t % gpr);
   if (row >= rows) return;
   long long m[16];
#pragma unroll
   for (int j = 0; j < 16; j++) m[j] = __double2ll_rn(ldexp(V[row * b + 16 * g + j], F - sh_e[16 * g + j]));
   for (int s = S - 1; s >= 0; s--) {
      u4 word = {0u, 0u, 0u, 0u};
#pragma unroll
      for (int j = 0; j < 16; j++) {
         const int d = (int)(signed char)(m[j] & 0xFF);
         m[j] = (m[j] - d) >> 8;
         word[j >> 2] |= ((uint32_t)d & 0xFFu) << (8 * (j & 3)); // byte j of the piece = column 16 g + j
      }
      *reinterpret_cast<u4 *>(Qrm + row * (uint64_t)(S * b) + s * b + 16 * g) = word;
   }
}

// One workgroup = TRG 16-row groups x all S b columns: the rows of a tile are one contiguous span of the row-major buffer, loaded
// with coalesced 16-byte reads into LDS (row stride S b + 16, 16 more per row group: the 16 lanes of a ds_read_b128 group then hit
// distinct banks); thread (row group fastest, slice, 16-column group) transposes a 16 x 16 byte block in registers and writes one
// 16-byte piece per column -- adjacent threads = adjacent row groups = contiguous bytes of the same operand row.
// The same pass can leave the scaled operand itself for the sparse gathers of the missing-call route (copy32: m 2^(1-F) in fp32, <= 4
// slices; copy64: m 2^(e_c - F)), rows < rows_valid: lane = (row, 4 resp. 2 columns) reads one dword / one halfword per slice from the
// LDS tile (conflict-free at the odd row stride) and writes 16 contiguous bytes -- a wave stores 1 KB runs.
__global__ __launch_bounds__(256) void k_unpack_slices(const int8_t *__restrict__ Qrm, uint64_t rows_pad, int b, int S, int TRG,
                                                        int8_t *__restrict__ Q, long long *__restrict__ colsum,
                                                        const unsigned long long *__restrict__ maxbits, uint64_t rows_valid,
                                                        float *__restrict__ copy32, double *__restrict__ copy64)
{
   __shared__ double sh_scale[64];
   extern __shared__ __attribute__((aligned(16))) unsigned char tile[];
   __shared__ int ssum[512];
   const int SB = S * b, rstr = SB + 16, gstr = 16 * rstr + 16, ncg = SB / 16; // bytes per row / LDS strides / 16-column groups
   const uint64_t rg0 = (uint64_t)blockIdx.x * TRG, groups = rows_pad / 16;
   const int ng = (int)(groups - rg0 < (uint64_t)TRG ? groups - rg0 : TRG);
   const u4 *src = reinterpret_cast<const u4 *>(Qrm + rg0 * 16 * (uint64_t)SB);
   for (int p = threadIdx.x; p < ng * 16 * ncg; p += 256) { // piece p: row p / ncg of the tile, 16-byte piece p % ncg
      const int row = p / ncg, pc = p % ncg;
      *reinterpret_cast<u4 *>(tile + (row >> 4) * gstr + (row & 15) * rstr + pc * 16) = src[p];
   }
   for (int t = threadIdx.x; t < 512; t += 256) ssum[t] = 0;
   if ((copy32 || copy64) && (int)threadIdx.x < b) {
      const int F = 8 * S - 2;
      sh_scale[threadIdx.x] = copy64 ? ldexp(1.0, slice_exponent(maxbits_fold(maxbits, threadIdx.x)) - F) : ldexp(1.0, 1 - F);
   }
   __syncthreads();
   if (copy32) { // thread = (row of the tile, group of 4 columns)
      const int per_row = b / 4;
      for (int t = threadIdx.x; t < ng * 16 * per_row; t += 256) {
         const int row = t / per_row, q = t % per_row;
         const uint64_t grow = rg0 * 16 + row;
         if (grow >= rows_valid) continue;
         const unsigned char *src_row = tile + (row >> 4) * gstr + (row & 15) * rstr + 4 * q;
         long long m[4] = {0, 0, 0, 0};
         for (int sl = 0; sl < S; sl++) {
            const uint32_t w = *reinterpret_cast<const uint32_t *>(src_row + sl * b);
#pragma unroll
            for (int j = 0; j < 4; j++) m[j] = m[j] * 256 + (long long)(signed char)((w >> (8 * j)) & 0xFFu);
         }
         float4 v;
         v.x = (float)((double)m[0] * sh_scale[4 * q]);
         v.y = (float)((double)m[1] * sh_scale[4 * q + 1]);
         v.z = (float)((double)m[2] * sh_scale[4 * q + 2]);
         v.w = (float)((double)m[3] * sh_scale[4 * q + 3]);
         *reinterpret_cast<float4 *>(copy32 + grow * b + 4 * q) = v;
      }
   }
   if (copy64) { // thread = (row of the tile, pair of columns)
      const int per_row = b / 2;
      for (int t = threadIdx.x; t < ng * 16 * per_row; t += 256) {
         const int row = t / per_row, q = t % per_row;
         const uint64_t grow = rg0 * 16 + row;
         if (grow >= rows_valid) continue;
         const unsigned char *src_row = tile + (row >> 4) * gstr + (row & 15) * rstr + 2 * q;
         long long m0 = 0, m1 = 0;
         for (int sl = 0; sl < S; sl++) {
            const uint32_t w = *reinterpret_cast<const unsigned short *>(src_row + sl * b);
            m0 = m0 * 256 + (long long)(signed char)(w & 0xFFu);
            m1 = m1 * 256 + (long long)(signed char)((w >> 8) & 0xFFu);
         }
         *reinterpret_cast<d2 *>(copy64 + grow * b + 2 * q) = (d2){(double)m0 * sh_scale[2 * q], (double)m1 * sh_scale[2 * q + 1]};
      }
   }
   for (int t = threadIdx.x; t < TRG * ncg; t += 256) {
      const int rg = t % TRG, cg = t / TRG; // column group cg = s * (b / 16) + g covers slice-columns 16 cg .. 16 cg + 15
      if (rg >= ng) continue;
      u4 piece[16];
#pragma unroll
      for (int i = 0; i < 16; i++) piece[i] = *reinterpret_cast<const u4 *>(tile + rg * gstr + i * rstr + cg * 16);
      int tot[16];
#pragma unroll
      for (int j = 0; j < 16; j++) { // column 16 cg + j: byte j of every piece, row i -> word i % 4, byte i / 4 (k_slice's order)
         u4 word = {0u, 0u, 0u, 0u};
         tot[j] = 0;
#pragma unroll
         for (int i = 0; i < 16; i++) {
            const uint32_t byte = (piece[i][j >> 2] >> (8 * (j & 3))) & 0xFFu;
            word[i & 3] |= byte << (8 * (i >> 2));
            tot[j] += (int)(signed char)byte;
         }
         *reinterpret_cast<u4 *>(Q + (uint64_t)(16 * cg + j) * rows_pad + (rg0 + rg) * 16) = word;
      }
      if (colsum) {
#pragma unroll
         for (int j = 0; j < 16; j++) atomicAdd(&ssum[16 * cg + j], tot[j]); // (LDS; |sum| <= 128 x 16 x TRG)
      }
   }
   if (colsum) {
      __syncthreads();
      for (int t = threadIdx.x; t < SB; t += 256)
         if (ssum[t])
            atomicAdd(reinterpret_cast<unsigned long long *>(&colsum[(blockIdx.x % I8_SHARDS) * I8_CS_STRIDE + t]), (unsigned long long)(long long)ssum[t]);
   }
}

__global__ __launch_bounds__(256) void k_dequant_rows(const int8_t *__restrict__ Qrm, uint64_t rows, int b, int S,
                                                       const unsigned long long *__restrict__ maxbits, float *__restrict__ copy32,
                                                       double *__restrict__ copy64)
{
   __shared__ double sh_scale[64];
   const int F = 8 * S - 2, gpr = b / 16;
   if ((int)threadIdx.x < b) sh_scale[threadIdx.x] = copy64 ? ldexp(1.0, slice_exponent(maxbits_fold(maxbits, threadIdx.x)) - F) : ldexp(1.0, 1 - F);
   __syncthreads();
   const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x, row = t / gpr;
   const int g = (int)(t % gpr);
   if (row >= rows) return;
   long long m[16];
#pragma unroll
   for (int j = 0; j < 16; j++) m[j] = 0;
   for (int s = 0; s < S; s++) { // slice 0 = top byte
      const u4 word = *reinterpret_cast<const u4 *>(Qrm + row * (uint64_t)(S * b) + s * b + 16 * g);
#pragma unroll
      for (int j = 0; j < 16; j++) m[j] = m[j] * 256 + (long long)(signed char)((word[j >> 2] >> (8 * (j & 3))) & 0xFFu);
   }
   // power-of-two scales: exact.  copy32: m 2^(1-F), |.| < 2, like k_slice's copy32; copy64: m 2^(e_c - F)
   if (copy32) {
#pragma unroll
      for (int q = 0; q < 4; q++) {
         float4 v;
         v.x = (float)((double)m[4 * q] * sh_scale[16 * g + 4 * q]);
         v.y = (float)((double)m[4 * q + 1] * sh_scale[16 * g + 4 * q + 1]);
         v.z = (float)((double)m[4 * q + 2] * sh_scale[16 * g + 4 * q + 2]);
         v.w = (float)((double)m[4 * q + 3] * sh_scale[16 * g + 4 * q + 3]);
         *reinterpret_cast<float4 *>(copy32 + row * b + 16 * g + 4 * q) = v;
      }
   }
   if (copy64) {
#pragma unroll
      for (int q = 0; q < 8; q++)
         *reinterpret_cast<d2 *>(copy64 + row * b + 16 * g + 2 * q) =
            (d2){(double)m[2 * q] * sh_scale[16 * g + 2 * q], (double)m[2 * q + 1] * sh_scale[16 * g + 2 * q + 1]};
   }
}

void i8_maxbits_fold(const unsigned long long *bits, double *out64, hipStream_t stream)
{
   hipLaunchKernelGGL(k_maxbits_fold, dim3(1), dim3(64), 0, stream, bits, out64);
   launch_check();
}
void i8_maxbits_set(const double *all, int G, unsigned long long *bits, hipStream_t stream)
{
   hipLaunchKernelGGL(k_maxbits_set, dim3(1), dim3(64), 0, stream, all, G, bits);
   launch_check();
}
void i8_slice_rows(const double *V, uint64_t rows, int b, int S, const SliceOp &op, int8_t *Qrm, hipStream_t stream)
{
   if (S > 8 || b > 64 || b % 16) throw Error(-1, "i8_slice_rows: S <= 8, b in {16, 32, 48, 64}");
   if (!rows) return;
   const uint64_t threads = rows * (b / 16);
   hipLaunchKernelGGL(k_slice_rows, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, stream, V, rows, b, S, gemm_i8_nsc_pad(S, b), op.maxbits, Qrm, op.colw);
   launch_check();
}
void i8_unpack_slices(const int8_t *Qrm, uint64_t rows_pad, int b, int S, const SliceOp &op, hipStream_t stream, uint64_t rows_valid, float *copy32,
                      double *copy64)
{
   const int SB = S * b;
   if (SB > 512 || SB % 16) throw Error(-1, "i8_unpack_slices: at most 512 slice-columns");
   const int trg = SB <= 128 ? 32 : SB <= 272 ? 16 : 8; // 16-row groups per workgroup: 41 / 74 / 68 KB of LDS at the largest S b of each class
   const uint64_t groups = rows_pad / 16;
   const size_t lds = (size_t)trg * (16 * (SB + 16) + 16);
   static bool attr_set = false;
   if (!attr_set) {
      (void)hipFuncSetAttribute(reinterpret_cast<const void *>(&k_unpack_slices), hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024);
      attr_set = true;
   }
   hipLaunchKernelGGL(k_unpack_slices, dim3((unsigned)((groups + trg - 1) / trg)), dim3(256), lds, stream, Qrm, rows_pad, b, S, trg, op.Q, op.colsum, op.maxbits,
                      rows_valid, copy32, copy64);
   launch_check();
}
void i8_dequant_rows(const int8_t *Qrm, uint64_t rows, int b, int S, const SliceOp &op, float *copy32, double *copy64, hipStream_t stream)
{
   if (!rows) return;
   const uint64_t threads = rows * (b / 16);
   hipLaunchKernelGGL(k_dequant_rows, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, stream, Qrm, rows, b, S, op.maxbits, copy32, copy64);
   launch_check();
}

// ------------------------------------------------------------------------------------------------
// K2i / K3i core:  acc[row][sc] = sum_k A[row][k] * Q[sc][k]  for A in {G.M, M}
//   `packed`: 2-bit records, one per output row (K2: the SNP-major stream, K = samples; K3: its sample-major copy,
//   K = SNPs).  TWO = false (K2): both integer matrices multiply the same operand Q.  TWO = true (K3): G.M multiplies
//   Qg (slices of T/sd), M multiplies Qm (slices of mean T/sd).
//   Workgroup = 4 waves, ONE wave per SIMD with the whole 512-register budget (up to 256 accumulator AGPRs), arranged
//   WR x WC; a wave owns MT x NT tiles of 32x32 of both matrices (2 MT NT <= 16 accumulators).  (Or 8 x 1 waves, two per SIMD with
//   256 registers each, around the same operand tiles -- the G.M-alone kernel at 512 rows, see I8Cfg and i8_tile_rows.)  Operand tiles
//   [WC NT 32 columns][KC k] are double-buffered (8 waves: three buffers, I8Cfg::NBUF) in LDS (row stride KC + 16 B: the 16 lanes of a ds_read_b128 group hit
//   distinct banks); the packed words go straight from global memory to the registers of the lane that decodes them.
//   Decode: a lane's dword w holds 16 codes; (w >> 2q) & 0x03030303 leaves codes q, q+4, q+8, q+12 in the four bytes
//   and v_perm_b32 with the code as selector looks G.M / M up in a 4-byte table -- 4 VALU ops per operand dword
//   pair; the Q bytes were stored in the matching order by k_slice.
//   Scheduling: with one wave per SIMD only the wave's own instruction order hides latency, and hipcc left alone
//   sinks every LDS read to just before its MFMAs and waits at once (measured: matrix pipe 42 % busy).  The loop body is
//   therefore a fixed pipeline of micro-steps (k-step, m-tile, n-group) fenced by sched_barrier(0), with explicit (asm)
//   loads and hand-counted s_waitcnt: the operand fragments of the next micro-step are read from LDS and its genotype
//   fragments decoded under this one's MFMAs, and the next chunk's global loads (first half of the chunk) and LDS
//   stores (second half) ride in the MFMA shadow instead of a burst at the chunk boundary.
//   Output: fp64 partials part[split * zblocks][row][mat][bw] (slices already recombined), summed by k_i8_combine.
template <int OFF>
__device__ __forceinline__ v4i lds_read16(uint32_t addr) // explicit LDS read: the caller places the s_waitcnt
{
   v4i r;
   asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(r) : "v"(addr), "n"(OFF));
   return r;
}
// NT: the load carries the `nt` bit -- served from L2 like any other, but its line is not kept in the CU's L1 on the way through (for a
// stream that a CU reads once: the packed words, I8Nt).  It counts in vmcnt like a plain load.
template <int OFF, bool NT = false>
__device__ __forceinline__ u4 gload16(const void *sbase, uint32_t voff) // explicit global load, address = sbase + voff + OFF
{
   u4 r;
   if constexpr (NT)
      asm volatile("global_load_dwordx4 %0, %1, %2 offset:%3 nt" : "=v"(r) : "v"(voff), "s"(sbase), "n"(OFF));
   else
      asm volatile("global_load_dwordx4 %0, %1, %2 offset:%3" : "=v"(r) : "v"(voff), "s"(sbase), "n"(OFF));
   return r;
}
__device__ __forceinline__ u2 gload8(const void *sbase, uint32_t voff) // ... 8 bytes, address = sbase + voff
{
   u2 r;
   asm volatile("global_load_dwordx2 %0, %1, %2" : "=v"(r) : "v"(voff), "s"(sbase));
   return r;
}
// hand-placed waits; the "+v" operands make the consumers of the loaded registers depend on the wait
__device__ __forceinline__ void lds_wait(v4i &a) { asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(a)); }
__device__ __forceinline__ void lds_wait(v4i &a, v4i &b) { asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(a), "+v"(b)); }
template <int N>
__device__ __forceinline__ void vm_wait(u4 &a)
{
   asm volatile("s_waitcnt vmcnt(%1)" : "+v"(a) : "n"(N));
}
template <int N>
__device__ __forceinline__ void vm_wait(u2 &a)
{
   asm volatile("s_waitcnt vmcnt(%1)" : "+v"(a) : "n"(N));
}
template <class F, int... I>
__device__ __forceinline__ void static_for_impl(F &&f, std::integer_sequence<int, I...>)
{
   (f(std::integral_constant<int, I>{}), ...);
}
template <int N, class F>
__device__ __forceinline__ void static_for(F &&f)
{
   static_for_impl(f, std::make_integer_sequence<int, N>{});
}

// MODE: how the missing-indicator matrix E is treated, chosen per shard from the genotype-code counts of K1
//   I8_FULL       both matrices, every block                                   (typical data, missing rate >~ 0.03 %)
//   I8_SKIP_EMPTY both matrices, but a 32 x 32 block of E without a missing genotype is skipped (wave-uniform branch): up
//                 to 23 % less time when nearly nothing is missing, ~10 % MORE when nothing can be skipped -- measured
//   I8_NO_MISSING the shard has no missing genotype at all (imputed / 1000-Genomes-like data): E = 0, only G.M is
//                 multiplied, M'Q = 1'Q comes from the column sums alone -- half the MFMAs
enum { I8_FULL = 0, I8_SKIP_EMPTY = 1, I8_NO_MISSING = 2 };

// What the main loop costs, measured with parts of it compiled out (profiles/r04_i8_ablation_2tile.txt; the 7-tile kernel in
// docs/history/DESIGN_r04.md §7c): the operand stream's L2 misses cost nothing, the packed words cost their HBM energy rather than
// their latency (issuing them further ahead ran slower), and at 7 tiles the per-chunk barrier costs nothing (under 8 waves it cost 150-170 cycles per chunk: I8Cfg::NBUF).  With an all-zero
// fp64 operand (same instructions, same traffic) the same launch takes 7.07 ms instead of 9.04: the kernel follows the bare MFMA
// stream's power curve.
// HALF: the last of the NT column tiles has only 16 columns (S b = 112 for b = 16, S = 7: 3.5 tiles).  As a 32-wide tile half
// of it would multiply zero padding -- an eighth of the kernel's MFMA passes; instead the 16 columns run on
// v_mfma_i32_16x16x64_i8, which takes TWO 32-k steps at once: the genotype fragments of an even and an odd k-step (lanes =
// 32 rows x 2 k-halves each) are regrouped by v_permlane16_swap into two 16-row x 64-k operands, the slice-column operand is
// one ds_read_b128 per lane with the matching (k-half, k-step) -> quarter order.  A bare stream of the two mixes
// (profiles/r03_mfma_mix_probe.txt): 3280 -> 3720 useful TOP/s.
// TILED: `packed` is in the band-tiled layout (kernels.hpp packed_piece_offset): the two 16-byte pieces of a lane are two loads in
// which the wave reads 1 KB contiguous each -- every 128-byte line of the packed stream is requested once.  On the row-major layout
// a load touches 32 lines and uses 32 bytes of each, and the other half of every line is wanted one chunk later, after the line has
// left the 32 KB L1: each packed byte crosses L2 -> L1 twice.  Same registers, same order of loads and waits.
template <bool TWO_, int MT_, int NT_, int WR_, int WC_, int KC_, int G_, int MODE_ = I8_FULL, bool HALF_ = false, bool TILED_ = false>
struct I8Cfg {
   static constexpr bool TWO = TWO_, HALF = HALF_, TILED = TILED_;
   static constexpr bool NT_P = false; // load policy of the packed words (issue_p): plain here, `nt` in the twin I8Nt makes of an instance
   static_assert(!TILED || KC_ == 256, "the band-tiled layout is cut in chunks of 256 codes");
   static constexpr int MT = MT_, NT = NT_, WR = WR_, WC = WC_, KC = KC_, G = G_, NQ = TWO ? 2 : 1, MODE = MODE_;
   static constexpr int MATS = MODE == I8_NO_MISSING ? 1 : 2;
   static constexpr int NTF = HALF ? NT - 1 : NT;       // full 32-column tiles
   static_assert(!(TWO && MATS == 1), "without E there is only one operand");
   // 8 waves (WR = 8): two waves per SIMD under ONE set of operand tiles -- 512 rows, the register budget of two co-resident
   // 4-wave workgroups, half their operand staging (the largest L2 -> L1 stream of the 4-wave kernel)
   static_assert((WR * WC == 4 || (WR == 8 && WC == 1)) && MATS * MT * NT <= 16 && (MT == 1 || G == 1) && G <= NT, "shape");
   static constexpr int WAVES = WR * WC, THREADS = 64 * WAVES;
   static_assert(!HALF || (WC == 1 && MT == 2 && G == 1 && MODE != I8_SKIP_EMPTY && (KC / 32) % 2 == 0), "half-tile variant");
   static constexpr int ROWS = WR * MT * 32;            // workgroup rows
   static constexpr int COLS = WC * NT * 32 - (HALF ? 16 : 0); // workgroup columns of each operand
   static constexpr int LDQ = KC + 16;                  // operand tile row stride (bytes)
   // HALF: the 16 rows of the remainder tile are read by ds_read_b128 with lanes l and l + 16 one 16-byte slot apart, which at
   // the odd slot pitch of the full tiles puts two lanes of a 16-lane service group on one slot (LDS bank conflicts 8.7 % of the
   // kernel's LDS cycles, round 4); those rows get an even pitch of 2 slots (mod 16) instead: slot = 2 j + (l >> 4 & 1)
   static constexpr int LDQH = LDQ + (HALF ? 16 : 0);   // row stride of the remainder tile's rows
   static constexpr int QTILE = COLS * LDQ + (HALF ? 16 * 16 : 0); // bytes of one operand tile
   static constexpr int STAGE = NQ * QTILE;
   // stage buffers.  8 waves: both waves of a SIMD stand at the chunk barrier together and nothing covers the cold start behind it (LDS
   // round trip + decode before the first MFMA), so a THIRD buffer lets a wave fetch the first operand fragment of chunk c + 1 BEFORE
   // the barrier that ends chunk c: the tile of c + 1 was stored during c - 1 and published one barrier ago, the barrier of c
   // publishes c + 2.  (One wave per SIMD, twice the MFMAs per chunk and wave: the barrier measured free -- two buffers.)
   static constexpr int NBUF = WR == 8 ? 3 : 2;
   static constexpr int SEGS = KC / 16, RSTEP = THREADS / SEGS; // 16-byte segments per row; rows covered by one piece of every thread
   // HALF with 512 threads: the 16 rows of the remainder tile are half a piece -- every thread takes 8 bytes of them instead
   // (512 x 8 B = 16 rows of KC = 256), so that all waves issue the same loads and count the same waits
   static constexpr bool HALF8 = HALF && RSTEP == 32;
   static constexpr int NP1 = HALF8 ? (COLS - 16) / RSTEP + 1 : COLS / RSTEP; // pieces per thread per operand tile
   static constexpr int NP = NQ * NP1;                  // ... per chunk
   static constexpr int KS = KC / 32;                   // 32-k steps per chunk
   static constexpr int PW = KC / 128;                  // 16-byte packed pieces per lane per m-tile (lane half = KC/2 k)
   static constexpr int NSTEP = KS * MT * G;            // micro-steps per chunk
   static constexpr int H = NSTEP / 2;
   // dynamic LDS: the NBUF operand tiles; the epilogue reuses it for WAVES x NT dumped tiles + the weights
   static constexpr int LDS_EPI = WAVES * NT * 4096 + 2 * WC * NT * 32 * 8;
   static constexpr int LDS_NEED = (NBUF * STAGE > LDS_EPI) ? NBUF * STAGE : LDS_EPI;
   // The narrowest column block (2 tiles: 136 registers, 34 KB) would fit three workgroups per CU; measured at 500,000 x
   // 100,000 (scripts/r4_narrow_probe.sh, GEMM kernels K2 / K3): three per CU 4.61 / 4.74 ms, two 4.31 / 4.39, one 5.20 / 5.74 --
   // so it asks for enough LDS to be two (the wider blocks are two or one by their registers: 224+ of 512).
   // (an 8-wave workgroup is alone on its CU by its waves: nothing to ask for)
   static constexpr int LDS_BYTES = (!TWO && NT <= 2 && WAVES == 4 && LDS_NEED < 56 * 1024) ? 56 * 1024 : LDS_NEED;
   static_assert((HALF8 ? (COLS - 16) % RSTEP == 0 && KC == 256 : COLS % RSTEP == 0) && NSTEP % 2 == 0 && LDS_BYTES <= 160 * 1024, "staging");
   static_assert(!HALF || RSTEP == 16 || HALF8, "the remainder tile is the last staging piece");
};

// The twin of instance C whose packed-word loads bypass L1: every packed byte is decoded by one lane of one wave, once per launch, and
// since the band tiling every line of the stream is requested once -- nothing of it is ever found in L1 again.  Same registers, same
// order of loads and waits, same bits.  (A wrapper and not one more argument of I8Cfg: the plain instances keep their names.)
// Measured at cfg3 (profiles/load_policy_ab.txt): the apply 10.26 -> 10.21 ms, the 4-slice apply 7.52 -> 7.40 ms, every run of six below
// every run of the parent.  The same bit on the operand pieces (staged once per workgroup, shared between CUs in L2) LOSES 0.17 / 0.82 ms,
// on the rows the missing-call gathers fetch 0.65 / 0.73 ms: neither is kept.
template <class C>
struct I8Nt : C {
   static constexpr bool NT_P = true;
};

// returns (MODE == I8_SKIP_EMPTY) whether any lane of the wave holds a missing genotype in this 32-row x 32-k block
// (wave-uniform), else true
template <int MODE>
__device__ __forceinline__ bool i8_decode(uint32_t w, v4i &ag, v4i &am, uint32_t tab1)
{
   // byte[code] of the two integer matrices: G.M (dosage, 0 if missing) and E = 1 - M (missing indicator): code 0 -> (2,0),
   // 1 (missing) -> (0,1), 2 -> (1,0), 3 -> (0,0).  E instead of M because E is almost all zeros; M'Q is recovered exactly in the
   // combine as 1'Q - E'Q.  What zeros and small bytes are worth depends on the PORT they enter the MFMA by (the bare stream,
   // profiles/mfma_ports_ab.txt section A, 2 waves per SIMD, TOP/s): random bytes on both ports 3340, zeros on both 4650; zeros on one
   // port alone already give 4420-4570 (zero A, random B) and 4600-4960 (random A, zero B); genotype bytes {0, 1, 2} against random
   // digits 3680-3710 with the genotypes on source A and 4310-4340 with them on source B.  So the fragments decoded here are the
   // SECOND operand of every MFMA of k_gemm_i8 and the slice-columns the first.
   // (the one-matrix kernel takes its table as an argument: G.M for the genotype products, E for the missing-indicator
   //  products of the SNPs whose missing calls are too many for the sparse route -- gemm_i8 `e_only`)
   const uint32_t tabG = MODE == I8_NO_MISSING ? tab1 : 0x00010002u, tabM = 0x00000100u;
#pragma unroll
   for (int q = 0; q < 4; q++) {
      const uint32_t sel = (w >> (2 * q)) & 0x03030303u;
      ag[q] = (int)__builtin_amdgcn_perm(0u, tabG, sel);
      if (MODE != I8_NO_MISSING) am[q] = (int)__builtin_amdgcn_perm(0u, tabM, sel);
   }
   if (MODE == I8_SKIP_EMPTY)
      return __builtin_amdgcn_ballot_w64(((w & ~(w >> 1)) & 0x55555555u) != 0u) != 0ull; // code 01: low bit set, high bit clear
   return true;
}

template <class C>
__global__ __launch_bounds__(C::THREADS, 1) void k_gemm_i8(const uint8_t *__restrict__ packed, size_t pitch,
                                                     const int8_t *__restrict__ Qg, const int8_t *__restrict__ Qm,
                                                     uint64_t k_pad, const double *__restrict__ wg, const double *__restrict__ wm, int bw,
                                                     double *__restrict__ part, uint64_t rows_pad, int chunks_total, int zb,
                                                     int nA, int sB, int cpsB, uint64_t rowB0, uint64_t rowsB, uint32_t tab1)
{
   constexpr bool TWO = C::TWO;
   constexpr int MODE = C::MODE, MATS = C::MATS;
   constexpr int MT = C::MT, NT = C::NT, NQ = C::NQ, KC = C::KC, NP = C::NP, NP1 = C::NP1, NSTEP = C::NSTEP, LDQ = C::LDQ,
                 H = C::H, G = C::G, PW = C::PW, NPK = MT * PW, NTF = C::NTF;
   constexpr bool HALF = C::HALF;
   constexpr int NBUF = C::NBUF;
   constexpr int AMASK = HALF ? 3 : 1; // decoded genotype fragments kept alive: 2, or 4 (even AND odd k-step of both m-tiles)
   extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
   const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
   const int li = lane & 31, kh = lane >> 5;
   const int wr = wave / C::WC, wc = wave % C::WC;
   // XCD-aware 1-D grid (workgroup w runs on XCD w % 8, each XCD has its own L2): the zb column blocks of a row tile
   // re-read the same packed rows, so they are given to the SAME XCD back to back (w and w + 8); the row tiles of one
   // split are dealt round-robin over the XCDs; splits are outermost, so that a round of workgroups streams one K range
   // of the operand in lock-step (nB is a multiple of 8, so the XCD of a phase-B workgroup is still w0 % 8).  (With the plain 3-D grid the column blocks ran a whole grid apart and K3 read the
   // packed stream from HBM twice: 29.9 GB per launch at cfg3 for 12.7 GB algorithmic.)
   //
   // Two-phase split-K.  Tile ids w0 (in the XCD-aware order) below nA -- whole rounds of one workgroup per CU -- run
   // UNSPLIT (phase A: no partial planes beyond plane 0, the whole round streams the operand in lock-step); the
   // remaining nB < #CU.. tiles, which would otherwise be a mostly idle last round, are cut sB ways along K (phase B,
   // workgroup ids nA + split * nB + k).  nA = 0 is plain split-K.
   // (8 waves: rows_pad is a multiple of 256, so the last 512-row tile may be half a tile -- see `idle`)
   const int rtiles = (int)((rows_pad + (C::WAVES == 8 ? C::ROWS - 1 : 0)) / C::ROWS), rtl = (rtiles + 7) / 8, ids = 8 * rtl * zb, nB = ids - nA;
   int w0 = blockIdx.x, split = 0, c_begin = 0, c_end = chunks_total;
   if (w0 >= nA) {
      const int wp = w0 - nA;
      split = wp / nB;
      w0 = nA + wp % nB;
      c_begin = split * cpsB;
      c_end = c_begin + cpsB < chunks_total ? c_begin + cpsB : chunks_total;
   }
   const int xcd = w0 & 7, sidx = w0 >> 3;
   const int zblk = sidx % zb, rt = (sidx / zb) * 8 + xcd;
   if (rt >= rtiles || c_begin >= c_end) return;
   const uint64_t row0 = (uint64_t)rt * C::ROWS;
   const int col0 = zblk * C::COLS;
   // 8 waves, last half tile: the waves whose rows lie behind rows_pad stage their share of the operand tiles and reach every barrier,
   // but load no packed words and write no partials (wave-uniform; never true with 4 waves)
   const bool idle = C::WAVES == 8 && __builtin_amdgcn_readfirstlane((int)(row0 + (uint64_t)(wr * 32 * MT) >= rows_pad)) != 0;

   v16i acc[MATS][MT][NT]; // [mat][m][n]   (HALF: the last n is never touched and costs nothing)
   v4i acch[MATS][MT][2];  // HALF: the 16-column remainder, rows 16 t .. 16 t + 15 of m-tile m in acch[mat][m][t]
#pragma unroll
   for (int a = 0; a < MATS; a++)
#pragma unroll
      for (int m = 0; m < MT; m++) acch[a][m][0] = acch[a][m][1] = (v4i){0, 0, 0, 0};
#pragma unroll
   for (int a = 0; a < MATS; a++)
#pragma unroll
      for (int m = 0; m < MT; m++)
#pragma unroll
         for (int n = 0; n < NT; n++)
#pragma unroll
            for (int r = 0; r < 16; r++) acc[a][m][n][r] = 0;

   // operand staging: piece r of this thread = operand r / NP1, row tid / SEGS + RSTEP (r % NP1), segment tid % SEGS
   const uint32_t qvoff = (uint32_t)((tid / C::SEGS) * k_pad + (tid % C::SEGS) * 16);
   const uint32_t lds_base = (uint32_t)(size_t)(__attribute__((address_space(3))) unsigned char *)smem;
   const int qdst = (tid / C::SEGS) * LDQ + (tid % C::SEGS) * 16;
   // packed words: lane (li, kh) of wave row wr decodes rows wr*32*MT + 32 m + li, k = (KC/2) kh + 16 ks .. of the chunk
   uint32_t pvoff[MT];
#pragma unroll
   for (int m = 0; m < MT; m++)
      pvoff[m] = C::TILED ? (uint32_t)(wr * MT * 32 * pitch + lane * 16) // band of the wave's first m-tile, piece (kh, li) of a 1 KB half block: the
                                                                           // band of m-tile m lies 32 m pitch further, on the scalar base (issue_p)
                          : (uint32_t)((wr * 32 * MT + 32 * m + li) * pitch + kh * (KC / 8));
   const uint8_t *prow = packed + row0 * pitch;
   const uint32_t aQ0 = lds_base + (uint32_t)(wc * 32 * NT + li) * LDQ + kh * (KC / 2);
   // HALF: lane (column j = lane & 15, quarter qd = lane >> 4) of the 16x16x64 operand reads k-half qd >> 1 of k-step 2 kp + (qd & 1)
   const uint32_t aQh0 = lds_base + (uint32_t)(32 * NTF * LDQ + (lane & 15) * C::LDQH) + ((lane >> 5) & 1) * (KC / 2) + ((lane >> 4) & 1) * 16;

   // (8 waves with the half tile: the remainder tile's 16 rows are one 8-byte piece per thread, row tid / 32, bytes 8 (tid % 32) ..)
   const uint32_t qvoffh = (uint32_t)((tid / 32) * k_pad + (tid % 32) * 8);
   const int qdsth = (tid / 32) * C::LDQH + (tid % 32) * 8;
   u4 qreg[NP];
   u2 qregh[NQ];
   u4 pk[MT][PW], pkn[MT][PW]; // packed words of the current / next chunk (one dword per k-step)

   auto issue_q = [&](auto rr, int cc) {
      constexpr int r = decltype(rr)::value, o = r / NP1, r1 = r % NP1;
      const int8_t *sb = ((TWO && o) ? Qm : Qg) + (uint64_t)(col0 + C::RSTEP * r1) * k_pad + (uint64_t)cc * KC;
      if constexpr (C::HALF8 && r1 == NP1 - 1)
         qregh[o] = gload8(sb, qvoffh);
      else
         qreg[r] = gload16<0>(sb, qvoff);
   };
   auto issue_p = [&](u4(&dst)[MT][PW], int cc) {
      const uint8_t *pb = prow + (size_t)cc * (C::TILED ? 2048 : KC / 4);
#pragma unroll
      for (int m = 0; m < MT; m++) {
         const uint8_t *pbm = C::TILED ? pb + (size_t)(32 * m) * pitch : pb;
         dst[m][0] = gload16<0, C::NT_P>(pbm, pvoff[C::TILED ? 0 : m]);
         if constexpr (PW == 2) dst[m][1] = gload16<(C::TILED ? 1024 : 16), C::NT_P>(pbm, pvoff[C::TILED ? 0 : m]);
      }
   };
   auto store_q = [&](auto rr, unsigned char *st, auto behind) { // `behind`: loads issued after the NP pieces (the packed words, or none)
      constexpr int r = decltype(rr)::value, o = r / NP1, r1 = r % NP1, NB = decltype(behind)::value;
      if constexpr (C::HALF8 && r1 == NP1 - 1) {
         vm_wait<NP - 1 - r + NB>(qregh[o]);
         *reinterpret_cast<u2 *>(st - qdst + qdsth + o * C::QTILE + r1 * C::RSTEP * LDQ) = qregh[o];
      } else {
         vm_wait<NP - 1 - r + NB>(qreg[r]); // loads are issued in the order q[0..NP), p[..]
         // (HALF: the last piece is the remainder tile's 16 rows, at their own pitch)
         const int hoff = (HALF && r1 == NP1 - 1) ? (tid / C::SEGS) * (C::LDQH - LDQ) : 0;
         *reinterpret_cast<u4 *>(st + o * C::QTILE + r1 * C::RSTEP * LDQ + hoff) = qreg[r];
      }
   };

   constexpr std::integral_constant<int, NPK> after_p{};
   constexpr std::integral_constant<int, 0> after_none{};
   // three buffers: the prologue stages chunks c_begin and c_begin + 1 (clamped, like every staged chunk, to the unit's last one)
   const int c_second = (c_begin + 1 < c_end) ? c_begin + 1 : c_begin;
   if (idle) {
      // the staging alone, chunk by chunk, barrier for barrier and buffer for buffer what the working waves do below
      static_for<NP>([&](auto rr) { issue_q(rr, c_begin); });
      static_for<NP>([&](auto rr) { store_q(rr, smem + qdst, after_none); });
      if constexpr (NBUF == 3) {
         asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); // the stores have read their registers
         static_for<NP>([&](auto rr) { issue_q(rr, c_second); });
         static_for<NP>([&](auto rr) { store_q(rr, smem + C::STAGE + qdst, after_none); });
      }
      __syncthreads();
      int wbuf = NBUF - 1; // buffer staged during the chunk: (c - c_begin + NBUF - 1) % NBUF
      for (int c = c_begin; c < c_end; c++) {
         const int cn = (c + NBUF - 1 < c_end) ? c + NBUF - 1 : c_end - 1;
         unsigned char *wst = smem + (size_t)wbuf * C::STAGE + qdst;
         static_for<NP>([&](auto rr) { issue_q(rr, cn); });
         static_for<NP>([&](auto rr) { store_q(rr, wst, after_none); });
         __syncthreads();
         wbuf = wbuf + 1 == NBUF ? 0 : wbuf + 1;
      }
   } else if constexpr (NBUF == 3) {
      // prologue: chunks c_begin and c_begin + 1
      static_for<NP>([&](auto rr) { issue_q(rr, c_begin); });
      static_for<NP>([&](auto rr) { store_q(rr, smem + qdst, after_none); });
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); // the stores have read their registers
      static_for<NP>([&](auto rr) { issue_q(rr, c_second); });
      issue_p(pk, c_begin);
      static_for<NP>([&](auto rr) { store_q(rr, smem + C::STAGE + qdst, after_p); });
#pragma unroll
      for (int m = 0; m < MT; m++)
#pragma unroll
         for (int h = 0; h < PW; h++) vm_wait<0>(pk[m][h]);
      __syncthreads();
   } else {
      // prologue: chunk c_begin
      static_for<NP>([&](auto rr) { issue_q(rr, c_begin); });
      issue_p(pk, c_begin);
      static_for<NP>([&](auto rr) { store_q(rr, smem + qdst, after_p); });
#pragma unroll
      for (int m = 0; m < MT; m++)
#pragma unroll
         for (int h = 0; h < PW; h++) vm_wait<0>(pk[m][h]);
      __syncthreads();
   }

   // micro-step s -> (ks, m, g); operand fragments are keyed by (ks, g), genotype fragments by (ks, m)
   constexpr int NG = (NT + G - 1) / G; // n-tiles per group (the last group may be shorter)
   v4i bq[2][NQ][NG];
   v4i bqh = {0, 0, 0, 0}, bqh2 = {0, 0, 0, 0}; // HALF: the 16-column operand(s) of the current pair of k-steps
   v4i ag[AMASK + 1], am[AMASK + 1]; // decoded genotype fragments, index = micro-step parity (HALF: (k-step parity, m))
   bool enz[AMASK + 1];             // ... and whether the E fragment has any nonzero at all (wave-uniform)
   constexpr std::integral_constant<int, 0> i0{};
   auto read_b = [&](auto kk, auto gg, auto par, uint32_t aQ, uint32_t aQ2, uint32_t aQh) { // the stage buffer's addresses
      constexpr int ks = decltype(kk)::value, g = decltype(gg)::value, p = decltype(par)::value;
      static_for<NG>([&](auto jj) {
         constexpr int j = decltype(jj)::value, n = g * NG + j;
         if constexpr (n < NTF) {
            bq[p][0][j] = lds_read16<32 * n * LDQ + ks * 16>(aQ);
            if constexpr (TWO) bq[p][NQ - 1][j] = lds_read16<32 * n * LDQ + ks * 16>(aQ2);
         }
      });
      if constexpr (HALF && (ks & 1) == 1) { // both k-steps of the pair in one read
         bqh = lds_read16<(ks >> 1) * 32>(aQh);
         if constexpr (TWO) bqh2 = lds_read16<(ks >> 1) * 32 + C::QTILE>(aQh);
      }
   };
   auto wait_b = [&](auto gg, auto par) {
      constexpr int g = decltype(gg)::value, p = decltype(par)::value;
      static_for<NG>([&](auto jj) {
         constexpr int j = decltype(jj)::value, n = g * NG + j;
         if constexpr (n < NTF) {
            if constexpr (TWO)
               lds_wait(bq[p][0][j], bq[p][NQ - 1][j]);
            else
               lds_wait(bq[p][0][j]);
         }
      });
      if constexpr (HALF) {
         if constexpr (TWO)
            lds_wait(bqh, bqh2);
         else
            lds_wait(bqh);
      }
   };
   // Three buffers: chunk c reads buffer i % 3 (i = c - c_begin), stages chunk min(c + 2, c_end - 1) into buffer (i + 2) % 3 -- the one
   // read during chunk c - 1, which every wave left before the barrier that ended c - 1 -- and, in its last micro-step, fetches the first
   // operand fragments of chunk c + 1 from buffer (i + 1) % 3 (stored during c - 1, published by that same barrier) and decodes its
   // first genotype fragment from the packed words that are one chunk ahead anyway: behind the barrier the first MFMAs find their
   // operands in registers.  The barrier that ends chunk c publishes the tile of c + 2 and says that every wave has left buffer i % 3,
   // which chunk c + 1 overwrites in its second half.  A clamped re-stage (the last two chunks of a unit; a unit of one chunk) lands in
   // a buffer that nobody reads any more; the fetch behind the last chunk reads a published buffer and is dropped.
   int buf = 0; // (three buffers: i % 3, stepped at the end of the chunk)
   if constexpr (NBUF == 3) {
      if (!idle) { // the first fragments of the first chunk
         read_b(i0, i0, i0, aQ0, aQ0 + C::QTILE, aQh0);
         enz[0] = i8_decode<MODE>(pk[0][0][0], ag[0], am[0], tab1);
         wait_b(i0, i0);
         __builtin_amdgcn_sched_barrier(0);
      }
   }
   for (int c = idle ? c_end : c_begin; c < c_end; c++) {
      if constexpr (NBUF == 2) buf = (c - c_begin) & 1;
      const int cn = (c + 1 < c_end) ? c + 1 : c; // the last chunk re-stages itself (branch-free pipeline)
      const uint32_t aQ = aQ0 + (uint32_t)buf * C::STAGE, aQ2 = aQ + C::QTILE;
      const int bufw = NBUF == 2 ? buf ^ 1 : (buf == 0 ? 2 : buf - 1), bufn = buf == NBUF - 1 ? 0 : buf + 1; // staged now; read next
      unsigned char *wst = smem + (size_t)bufw * C::STAGE + qdst;
      const int cq = NBUF == 2 ? cn : ((c + 2 < c_end) ? c + 2 : c_end - 1); // the chunk whose operand tile is staged
      const uint32_t aQh = aQh0 + (uint32_t)buf * C::STAGE;
      if constexpr (NBUF == 2) {
         if constexpr (HALF) bqh = bqh2 = (v4i){0, 0, 0, 0};
         read_b(i0, i0, i0, aQ, aQ2, aQh);
         enz[0] = i8_decode<MODE>(pk[0][0][0], ag[0], am[0], tab1);
         wait_b(i0, i0);
         __builtin_amdgcn_sched_barrier(0);
      }

      static_for<NSTEP>([&](auto ss) {
         constexpr int s = decltype(ss)::value;
         constexpr int ks = s / (MT * G), m = (G == 1) ? s % MT : 0, g = (G == 1) ? 0 : s % G;
         constexpr int bkey = ks * G + g, akey = ks * MT + m;
         constexpr bool last = (s + 1 == NSTEP);
         constexpr int s1 = last ? s : s + 1;
         constexpr int ks1 = s1 / (MT * G), m1 = (G == 1) ? s1 % MT : 0, g1 = (G == 1) ? 0 : s1 % G;
         constexpr int bkey1 = ks1 * G + g1, akey1 = ks1 * MT + m1;
         // --- staging of chunk cn: loads in the first half, packed words at the half-way mark, LDS stores in the second
         if constexpr (s < H) {
            static_for<(s + 1) * NP / H - s * NP / H>([&](auto jj) {
               issue_q(std::integral_constant<int, s * NP / H + decltype(jj)::value>{}, cq);
            });
         }
         if constexpr (s == H - 1) issue_p(pkn, cn);
         if constexpr (s >= H) {
            static_for<(s - H + 1) * NP / H - (s - H) * NP / H>([&](auto jj) {
               store_q(std::integral_constant<int, (s - H) * NP / H + decltype(jj)::value>{}, wst, after_p);
            });
         }
         // --- operand fragments of the next micro-step
         if constexpr (bkey1 != bkey)
            read_b(std::integral_constant<int, ks1>{}, std::integral_constant<int, g1>{}, std::integral_constant<int, (bkey1 & 1)>{}, aQ, aQ2, aQh);
         // (three buffers, last micro-step: the packed words of the next chunk have had half a chunk to arrive; fragment registers
         // bq[0] and ag[0] / am[0] were last used one k-step ago)
         constexpr bool ahead = NBUF == 3 && last;
         if constexpr (ahead) {
            static_assert(G == 1 && ((NSTEP / MT - 1) & 1) == 1 && ((NSTEP - 1) & AMASK) != 0, "the last micro-step leaves bq[0] and ag[0] free");
#pragma unroll
            for (int mm = 0; mm < MT; mm++)
#pragma unroll
               for (int h = 0; h < PW; h++) {
                  vm_wait<0>(pkn[mm][h]);
                  pk[mm][h] = pkn[mm][h];
               }
            read_b(i0, i0, i0, aQ0 + (uint32_t)bufn * C::STAGE, aQ0 + (uint32_t)bufn * C::STAGE + C::QTILE, aQh0);
         }
         // --- this micro-step's MFMAs, the next micro-step's decode in their shadow
         static_for<NG>([&](auto jj) {
            constexpr int j = decltype(jj)::value, n = g * NG + j;
            if constexpr (n < NTF) {
               acc[0][m][n] = __builtin_amdgcn_mfma_i32_32x32x32_i8(bq[bkey & 1][0][j], ag[akey & AMASK], acc[0][m][n], 0, 0, 0);
               if constexpr (MODE == I8_FULL)
                  acc[1][m][n] = __builtin_amdgcn_mfma_i32_32x32x32_i8(bq[bkey & 1][NQ - 1][j], am[akey & AMASK], acc[1][m][n], 0, 0, 0);
            }
            if constexpr (j == 0 && akey1 != akey)
               enz[akey1 & AMASK] = i8_decode<MODE>(pk[m1][ks1 >> 2][ks1 & 3], ag[akey1 & AMASK], am[akey1 & AMASK], tab1);
            if constexpr (j == 0 && ahead) enz[0] = i8_decode<MODE>(pk[0][0][0], ag[0], am[0], tab1);
         });
         if constexpr (HALF && (ks & 1) == 1) {
            // the 16 remaining columns over k-steps ks - 1 and ks: row group r of the even / odd fragment = rows 16 (r & 1) ..
            // of k-half r >> 1; v_permlane16_swap exchanges row groups 1, 3 of its first operand with 0, 2 of its second, which
            // leaves [even.0, odd.0, even.2, odd.2] (rows 0..15 in all four k quarters) and [even.1, odd.1, even.3, odd.3]
            v4i t0 = ag[m], t1 = ag[2 + m];
#pragma unroll
            for (int q = 0; q < 4; q++) {
               const auto r = __builtin_amdgcn_permlane16_swap((unsigned)t0[q], (unsigned)t1[q], false, false);
               t0[q] = (int)r[0];
               t1[q] = (int)r[1];
            }
            acch[0][m][0] = __builtin_amdgcn_mfma_i32_16x16x64_i8(bqh, t0, acch[0][m][0], 0, 0, 0);
            acch[0][m][1] = __builtin_amdgcn_mfma_i32_16x16x64_i8(bqh, t1, acch[0][m][1], 0, 0, 0);
            if constexpr (MATS == 2) { // the missing-indicator matrix against its own operand (K3) or the same one (K2)
               v4i u0 = am[m], u1 = am[2 + m];
#pragma unroll
               for (int q = 0; q < 4; q++) {
                  const auto r = __builtin_amdgcn_permlane16_swap((unsigned)u0[q], (unsigned)u1[q], false, false);
                  u0[q] = (int)r[0];
                  u1[q] = (int)r[1];
               }
               acch[1][m][0] = __builtin_amdgcn_mfma_i32_16x16x64_i8(TWO ? bqh2 : bqh, u0, acch[1][m][0], 0, 0, 0);
               acch[1][m][1] = __builtin_amdgcn_mfma_i32_16x16x64_i8(TWO ? bqh2 : bqh, u1, acch[1][m][1], 0, 0, 0);
            }
         }
         if constexpr (MODE == I8_SKIP_EMPTY) {
            if (enz[akey & AMASK]) {
               static_for<NG>([&](auto jj) {
                  constexpr int j = decltype(jj)::value, n = g * NG + j;
                  if constexpr (n < NT)
                     acc[1][m][n] = __builtin_amdgcn_mfma_i32_32x32x32_i8(bq[bkey & 1][NQ - 1][j], am[akey & AMASK], acc[1][m][n], 0, 0, 0);
               });
            }
         }
         __builtin_amdgcn_sched_barrier(0);
         if constexpr (bkey1 != bkey) {
            wait_b(std::integral_constant<int, g1>{}, std::integral_constant<int, (bkey1 & 1)>{});
            __builtin_amdgcn_sched_barrier(0);
         }
         if constexpr (ahead) { // lgkmcnt(0): the fetched fragments are here AND this wave's stores of the chunk are in LDS
            wait_b(i0, i0);
            __builtin_amdgcn_sched_barrier(0);
         }
      });
      if constexpr (NBUF == 3) {
         // every load of the chunk has been waited for (the packed words last) and lgkmcnt is zero: the bare barrier, without the
         // vmcnt(0) lgkmcnt(0) that __syncthreads() puts in front of it
         asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
         __builtin_amdgcn_s_barrier();
         asm volatile("" ::: "memory");
         __builtin_amdgcn_sched_barrier(0);
         buf = bufn;
      } else {
#pragma unroll
         for (int m = 0; m < MT; m++)
#pragma unroll
            for (int h = 0; h < PW; h++) {
               vm_wait<0>(pkn[m][h]);
               pk[m][h] = pkn[m][h];
            }
         __syncthreads();
      }
   }

   // epilogue: the slices are recombined here, per split and column block, into fp64 partial sums -- virtual column
   // j = sc mod bw (bw = lcm(32, b): slice-column sc = s*b + c lands on j == c mod b), so a row of partials is
   // 2 x bw doubles instead of 2 x S*b int32.  Every product w * acc is exact (w is a power of two, |acc| < 2^31); only
   // the additions round, last slice (smallest terms) first.
   const int tile0 = (col0 + wc * 32 * NT) / 32;
   // partial planes: plane 0 holds every row, planes 1 .. sB-1 only the rows of the phase-B tiles (rows >= rowB0)
   double *out = (split == 0 ? part + (((size_t)zblk * rows_pad + row0 + wr * 32 * MT) * 2) * bw
                             : part + (size_t)zb * rows_pad * 2 * bw +
                                  ((((size_t)(split - 1) * zb + zblk) * rowsB + (row0 - rowB0) + wr * 32 * MT) * 2) * bw) +
                 (size_t)li * 2 * bw + 16 * kh; // lane (li, kh): row li of the m-tile, columns 16 kh .. of the 32-column tile
   //
   // Register discipline: the 256 accumulators own every AGPR, and reading ONE element of an AGPR-resident 16-vector makes
   // the compiler copy the whole vector to VGPRs, so any epilogue that walks rows across tiles keeps hundreds of extra
   // VGPRs alive and the allocator answers by spilling INSIDE the main loop (measured: 10 scratch stores per chunk,
   // 3.5 GB of spill traffic per launch, matrix pipe 48 % busy).  So the tiles are dumped to LDS one at a time (the operand
   // tiles are dead by now; 4 KB per tile and wave) and the recombination runs from LDS with a handful of registers.
   //
   // The slice-columns are the MFMAs' FIRST operand and the genotype rows their second (source B is the port whose bytes cost the
   // power -- DESIGN.md 3a, "Which port carries the digits"), so an accumulator tile is the TRANSPOSE of the tile of partials:
   // register r of lane (li, kh) is column (r & 3) + 8 (r >> 2) + 4 kh of genotype row li.  The dump keeps the addresses it had
   // with the operands the other way round (conflict-free), so the tile lies in LDS as [column][row]; a lane recombines half a
   // row of partials and writes it as one whole 128-byte line, 16 bytes at a time: L2 puts the line together.
   __syncthreads(); // every wave has finished reading the operand tiles
   constexpr int WREG = NT * 4096; // bytes of a wave's private tile area: [NT][32 cols][32 rows] int32
   double *sW = reinterpret_cast<double *>(smem + C::WAVES * WREG); // weights of this workgroup's slice-columns: [2][COLS]
   constexpr int WCOLS = C::WC * NT * 32; // (HALF: the 16 columns missing from the last tile carry zero weights)
   for (int t = tid; t < WCOLS; t += C::THREADS) {
      sW[t] = t < C::COLS ? wg[col0 + t] : 0.0;
      sW[WCOLS + t] = t < C::COLS ? wm[col0 + t] : 0.0;
   }
   __syncthreads();
   static_assert(C::LDS_BYTES >= C::WAVES * WREG + 2 * WCOLS * 8, "epilogue LDS layout");
   if (idle) return; // (behind the last barrier)
   int *sT = reinterpret_cast<int *>(smem + wave * WREG);
   const double *sWl = sW + wc * 32 * NT + 16 * kh;
   const int kb = bw / 32; // tiles n, n + kb, ... feed the same 32 virtual columns, 32 ((tile0 + n) % kb) ..
#pragma unroll
   for (int a = 0; a < MATS; a++) // (the E plane of the partials is not written in I8_NO_MISSING mode: the combine knows)
#pragma unroll
      for (int m = 0; m < MT; m++) {
#pragma unroll
         for (int n = 0; n < NTF; n++) {
            const v16i v = acc[a][m][n];
#pragma unroll
            for (int r = 0; r < 16; r++) sT[(n * 32 + (r & 3) + 8 * (r >> 2) + 4 * kh) * 32 + li] = v[r];
            __builtin_amdgcn_sched_barrier(0);
         }
         if constexpr (HALF) { // 16x16 C/D map: register r of lane l = column 4 (l >> 4) + r of row l & 15 of row half t; columns 16..31 of the tile are zero
#pragma unroll
            for (int t = 0; t < 2; t++)
#pragma unroll
               for (int r = 0; r < 4; r++) {
                  const int col = 4 * (lane >> 4) + r;
                  sT[(NTF * 32 + col) * 32 + 16 * t + (lane & 15)] = acch[a][m][t][r];
                  sT[(NTF * 32 + 16 + col) * 32 + 16 * t + (lane & 15)] = 0;
               }
         }
         __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
         __builtin_amdgcn_wave_barrier();
         // lane (li, kh) recombines columns 16 kh .. 16 kh + 15 of row li, two at a time (the weight goes by the column)
         for (int j = 0; j < 16; j += 2) {
            const int col = 16 * kh + j;
            for (int k = 0; k < kb; k++) {
               double acc0 = 0.0, acc1 = 0.0;
               for (int n = NT - 1 - ((NT - 1 - k) % kb); n >= 0; n -= kb) { // tiles n == k (mod kb), last slice first
                  acc0 += sWl[a * WCOLS + 32 * n + j] * (double)sT[(n * 32 + col) * 32 + li];
                  acc1 += sWl[a * WCOLS + 32 * n + j + 1] * (double)sT[(n * 32 + col + 1) * 32 + li];
               }
               *reinterpret_cast<double2 *>(&out[((size_t)(32 * m) * 2 + a) * bw + 32 * ((tile0 + k) % kb) + j]) = make_double2(acc0, acc1);
            }
         }
         __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
         __builtin_amdgcn_wave_barrier();
      }
}

// sum of the per-split / per-column-block fp64 partials, fold of the virtual columns (j == c mod b), M'Q = 1'Q - E'Q,
// and the per-row standardisation:
//   K2 (mean != null): out[row][c] = ( G[row][c] - mean[row] M[row][c] ) / sd[row]   (0 if sd <= 1e-9)
//   K3               : out[row][c] =   G[row][c] - M[row][c]
// The K2 flavour can also leave the column maxima of out * rs0 and out * rs1 behind (the two K3 operands), which saves
// the next stage a pass over T.
__global__ __launch_bounds__(256) void k_i8_combine(const double *__restrict__ part, int zb, int rows_tile, int nA, int sB, uint64_t rowB0,
                                                     uint64_t rowsB, uint64_t rows_pad, uint64_t rows_valid, int mats,
                                                     const double *__restrict__ eplane /* [rows_pad][b]: E'Q from the sparse path */,
                                                     int b, int bw, int S,
                                                     const double *__restrict__ wm, const long long *__restrict__ colsum_m /* 1'Qm */,
                                                     const double *__restrict__ mean, const double *__restrict__ sd,
                                                     double *__restrict__ out, const double *__restrict__ rs0,
                                                     unsigned long long *__restrict__ bits0, const double *__restrict__ rs1,
                                                     unsigned long long *__restrict__ bits1)
{
   __shared__ double smax[256], sw[9 * 64], sones[64];
   const int c = threadIdx.x % b, r_in = threadIdx.x / b, r_step = 256 / b;
   double m0 = 0.0, m1 = 0.0;
   // 1'Qm recombined once per block: sum_s w[s,c] colsum[s,c] (shards folded), small terms first
   // (mats == -1: the plain product of ONE integer matrix -- out = sum of its partials, rows >= rows_valid zero)
   for (int t = threadIdx.x; t < S * b; t += 256) sw[t] = (mats < 0 || !colsum_m) ? 0.0 : wm[t] * (double)colsum_fold(colsum_m, t);
   __syncthreads();
   if ((int)threadIdx.x < b) {
      double o = 0.0;
      for (int s = S - 1; s >= 0; s--) o += sw[s * b + threadIdx.x];
      sones[threadIdx.x] = o;
   }
   __syncthreads();
   if (r_in < r_step) {
      const double ones = sones[c];
      for (uint64_t row = (uint64_t)blockIdx.x * r_step + r_in; row < rows_pad; row += (uint64_t)gridDim.x * r_step) {
         double accg = 0.0, acce = 0.0;
         const int rt = (int)(row / rows_tile);
         for (int z = 0; z < zb; z++) {
            const int w0 = ((rt >> 3) * zb + z) * 8 + (rt & 7);
            const int np = w0 < nA ? 1 : sB; // phase-A tiles were not split
            for (int p = 0; p < np; p++) {
               const double *q = p == 0 ? part + (((size_t)z * rows_pad + row) * 2) * bw
                                        : part + (size_t)zb * rows_pad * 2 * bw + ((((size_t)(p - 1) * zb + z) * rowsB + (row - rowB0)) * 2) * bw;
               for (int j = c; j < bw; j += b) {
                  accg += q[j];
                  if (mats == 2) acce += q[bw + j];
               }
            }
         }
         // (mats == 1: E is not in the partials -- it is zero, or comes from the sparse path; the padding rows are all
         // "missing" and must stay zero)
         if (mats == 1) acce = row >= rows_valid ? ones : (eplane ? eplane[row * b + c] : 0.0);
         const double accm = ones - acce;
         double v;
         if (mats < 0)
            v = row < rows_valid ? accg : 0.0;
         else if (mean) {
            const double sdv = sd[row];
            v = (sdv > 1e-9) ? (accg - mean[row] * accm) / sdv : 0.0;
         } else
            v = accg - accm;
         out[row * b + c] = v;
         if (bits0) {
            m0 = fmax(m0, fabs(v * rs0[row]));
            m1 = fmax(m1, fabs(v * rs1[row]));
         }
      }
   }
   if (bits0) {
      colmax_commit(m0, b, smax, bits0);
      colmax_commit(m1, b, smax, bits1);
   }
}

// ---- the instances ----
// Every k_gemm_i8<I8Cfg<...>> there is, once.  The shape rules below ask this list what exists, gemm_i8 looks its kernel up in it, and
// the static_assert behind i8_shape_static refuses to compile a shape without an instance.  All are KC = 256, waves WR x 1.
template <class... C>
struct I8List {};
constexpr bool I8_RM = false, I8_TL = true; // layout of `packed`: row-major / band-tiled (I8Cfg::TILED)
constexpr bool I8_HALF = true;
// two operands (K3): 64-row waves
template <int NT, int MODE, bool TILED, bool HALF = false>
using I8Two = I8Cfg<true, 2, NT, 4, 1, 256, 1, MODE, HALF, TILED>;
// one operand, G.M alone (I8_NO_MISSING): 64-row waves, 4 of them or 8
template <int NT, bool TILED, bool HALF = false, int WR = 4>
using I8One = I8Cfg<false, 2, NT, WR, 1, 256, 1, I8_NO_MISSING, HALF, TILED>;
// one operand, both matrices (K2, dense missing-indicator routes), row-major only: 64-row waves in a narrow column block (<= 3 tiles) and
// for the half tile; from 4 tiles up 32-row waves, the tiles in 2 groups
template <int NT, int MODE, bool HALF = false>
using I8Both = I8Cfg<false, (NT <= 3 || HALF) ? 2 : 1, NT, 4, 1, 256, (NT <= 3 || HALF) ? 1 : 2, MODE, HALF, I8_RM>;
using I8Instances = I8List<
   I8Two<2, I8_FULL, I8_RM>, I8Two<3, I8_FULL, I8_RM>, I8Two<4, I8_FULL, I8_RM>, I8Two<4, I8_FULL, I8_RM, I8_HALF>,
   I8Two<2, I8_FULL, I8_TL>, I8Two<3, I8_FULL, I8_TL>, I8Two<4, I8_FULL, I8_TL>, I8Two<4, I8_FULL, I8_TL, I8_HALF>,
   I8Two<2, I8_SKIP_EMPTY, I8_RM>, I8Two<3, I8_SKIP_EMPTY, I8_RM>, I8Two<4, I8_SKIP_EMPTY, I8_RM>,
   I8Two<2, I8_SKIP_EMPTY, I8_TL>, I8Two<3, I8_SKIP_EMPTY, I8_TL>, I8Two<4, I8_SKIP_EMPTY, I8_TL>,
   I8One<2, I8_RM>, I8One<3, I8_RM>, I8One<4, I8_RM>, I8One<5, I8_RM>, I8One<6, I8_RM>, I8One<7, I8_RM>, I8One<8, I8_RM>,
   I8One<2, I8_TL>, I8One<3, I8_TL>, I8One<4, I8_TL>, I8One<5, I8_TL>, I8One<6, I8_TL>, I8One<7, I8_TL>, I8One<8, I8_TL>,
   I8One<2, I8_RM, I8_HALF>, I8One<4, I8_RM, I8_HALF>, I8One<2, I8_TL, I8_HALF>, I8One<4, I8_TL, I8_HALF>,
   I8One<2, I8_RM, false, 8>, I8One<4, I8_RM, I8_HALF, 8>, I8One<2, I8_TL, false, 8>, I8One<4, I8_TL, I8_HALF, 8>, // 512 rows
   I8Both<2, I8_FULL>, I8Both<3, I8_FULL>, I8Both<4, I8_FULL>, I8Both<5, I8_FULL>, I8Both<6, I8_FULL>, I8Both<7, I8_FULL>, I8Both<8, I8_FULL>,
   I8Both<4, I8_FULL, I8_HALF>,
   I8Both<2, I8_SKIP_EMPTY>, I8Both<3, I8_SKIP_EMPTY>, I8Both<4, I8_SKIP_EMPTY>, I8Both<5, I8_SKIP_EMPTY>, I8Both<6, I8_SKIP_EMPTY>,
   I8Both<7, I8_SKIP_EMPTY>, I8Both<8, I8_SKIP_EMPTY>,
   // the L1-bypassing twins (I8Nt) of what the headline and the cheap pass launch: G.M alone, band-tiled, 3.5 tiles at 512 and 256 rows
   // and 2 tiles at 256 rows
   I8Nt<I8One<4, I8_TL, I8_HALF, 8>>, I8Nt<I8One<4, I8_TL, I8_HALF>>, I8Nt<I8One<2, I8_TL>>>;

// what tells two instances apart: the operands, the matrices, the column block, the tile height, the layout of `packed` and the policy
// of its loads
struct I8Key {
   bool two;
   int mode, nt;
   bool half;
   int rows;
   bool tiled;
   bool nt_p = false;
};
// f(C{}) for the instance C with this key, and its answer; false if there is none
template <class... C, class F>
constexpr bool i8_find(I8List<C...>, const I8Key &k, F &&f)
{
   return ((k.two == C::TWO && k.mode == C::MODE && k.nt == C::NT && k.half == C::HALF && k.rows == C::ROWS && k.tiled == C::TILED &&
            k.nt_p == C::NT_P && f(C{})) || ...);
}
// the key of every member of the list, in the list's order (fpca_debug_i8_instances: what a census of the launched instances is held to).
// The L1-bypassing twins are not listed: they share their plain twin's six numbers, and tests/test_gpu_load_policy.py launches each
template <class... C>
static int i8_keys(I8List<C...>, int (*out)[6], int cap)
{
   const I8Key keys[] = {I8Key{C::TWO, C::MODE, C::NT, C::HALF, C::ROWS, C::TILED, C::NT_P}...};
   int n = 0;
   for (const I8Key &key : keys) {
      if (key.nt_p) continue;
      if (n < cap) {
         const int k[6] = {key.two, key.mode, key.nt, key.half, key.rows, key.tiled};
         std::copy(k, k + 6, out[n]);
      }
      n++;
   }
   return n;
}
int gemm_i8_instances(int (*out)[6], int cap) { return i8_keys(I8Instances{}, out, cap); }

constexpr bool i8_exists(bool two, int mode, int nt, bool half, int rows, bool tiled)
{
   return i8_find(I8Instances{}, I8Key{two, mode, nt, half, rows, tiled}, [](auto) { return true; });
}
// tile height of the 4-wave instance of (two, mode, nt, half), whatever the layout; 0: there is none
constexpr int i8_rows4(bool two, int mode, int nt, bool half)
{
   for (int rows = 256; rows >= 128; rows -= 128)
      if (i8_exists(two, mode, nt, half, rows, I8_RM) || i8_exists(two, mode, nt, half, rows, I8_TL)) return rows;
   return 0;
}

// ---- shape selection ----
// The slice-columns (S*b, rounded up to whole 32-column tiles) are cut into `zb` equal column blocks of NT tiles
// (blockIdx.z); 4 x 1 waves per workgroup, KC = 256:
//   K2: wave = 32 rows x NT <= 8 tiles (every packed row is decoded exactly once; any S without padding for b = 32)
//   K3: wave = 64 rows x NT = 3..4 tiles of BOTH operands (two operand tiles per stage -> half the columns per block)
// ... or 8 x 1 waves of 64 rows (512-row tiles) for the G.M-alone kernel at 3.5 and at 2 tiles, where two 4-wave workgroups share a
// CU anyway and each stages its own copy of the operand tile: i8_tile_rows decides per launch.
// Measured alternatives at cfg3, S = 8 (K2 / K3 ms): 2 x 2 waves of 64 x 128 | 128 x 64: 19.2 / 22.4; K3 with 32-row waves,
// all tiles and KC = 128: 24.3; K2 with the K3 shape: 18.9 -- versus 18.7 / 20.6 for the shapes kept.
struct I8Shape {
   int nt, zb, rows, cols, kc;
   bool half; // the last tile is the 16-column remainder (v_mfma_i32_16x16x64_i8), cols = 32 nt - 16
   bool wide; // an 8-wave instance (512 rows) of this shape exists
};

static int i8_ncu()
{
   static int ncu = 0;
   if (!ncu) {
      // FPCA_I8_NCU (test builds): the CU count to plan for, a multiple of 8 -- the two-phase regime at a few thousand rows.  The
      // grid then exceeds or undercuts the device's CUs, which the kernel does not depend on
      if (const char *env_n = FPCA_TEST_ENV("FPCA_I8_NCU")) {
         const int n = atoi(env_n);
         if (n < 8 || n % 8) throw Error(-1, "FPCA_I8_NCU is a multiple of 8, at least 8");
         ncu = n;
      } else {
         hipDeviceProp_t prop;
         int dev = 0;
         (void)hipGetDevice(&dev);
         ncu = (hipGetDeviceProperties(&prop, dev) == hipSuccess && prop.multiProcessorCount >= 8) ? prop.multiProcessorCount / 8 * 8 : 256;
      }
   }
   return ncu;
}

// Tile height of one launch: 512 rows (8 waves under one operand tile) where the instance exists, rows_pad is whole 256-row units (the
// last 512-row tile may then be half a tile; the row ranges of the chunked all-reduce need not be) and the launch has at least
// I8_WIDE_QUARTERS / 4 rounds of 512-row tiles.  Measured at cfg3 on 256 CUs (profiles/wide_ab.txt): K3, 977 tiles, 5.41 -> 5.28 ms;
// K2, 196 tiles (3/4 of a round, plain split-K), 5.30 -> 5.25 ms -- and the apply with both 0.11 ms below the apply with K3 alone,
// every run of six: three quarters of a round it is.  The 2-tile instance (4-slice passes) is slower than its 4-wave twin (K3 3.76 ->
// 3.91 ms) and never chosen.  FPCA_I8_ROWS=256|512 (test
// builds) forces the choice wherever an instance exists.
constexpr int I8_WIDE_QUARTERS = 3;
static int i8_tile_rows(uint64_t rows_pad, int ncu, const I8Shape &sh)
{
   if (!sh.wide || !rows_pad || rows_pad % 256) return sh.rows;
   static const char *env_r = FPCA_TEST_ENV("FPCA_I8_ROWS");
   if (env_r) {
      const int r = atoi(env_r);
      if (r != 256 && r != 512) throw Error(-1, "FPCA_I8_ROWS is 256 or 512");
      return r == 512 ? 512 : sh.rows;
   }
   const uint64_t tiles512 = (rows_pad + 511) / 512;
   return (sh.half && sh.nt == 4 && tiles512 * 4 >= (uint64_t)I8_WIDE_QUARTERS * ncu) ? 512 : sh.rows;
}

// Load policy of one launch: the packed words bypass L1 wherever the instance has a twin that does (I8Nt).  The e_only launches on the
// hybrid route's compacted records stay plain, and so does every instance without a twin.  FPCA_I8_LOADS=plain|p (test builds) forces
// the choice wherever a twin exists.
static bool i8_nt_p(I8Key k, bool e_only)
{
   static const char *env_l = FPCA_TEST_ENV("FPCA_I8_LOADS");
   if (env_l && std::strcmp(env_l, "p") && std::strcmp(env_l, "plain")) throw Error(-1, "FPCA_I8_LOADS is plain or p");
   if (e_only || (env_l && !std::strcmp(env_l, "plain"))) return false;
   k.nt_p = true;
   return i8_find(I8Instances{}, k, [](auto) { return true; });
}

// the 4-wave shape, whatever the launch and the device
constexpr I8Shape i8_shape_static(int S, int b, bool two, int mode)
{
   const int tiles = (S * b + 31) / 32, cap = two ? 4 : 8; // largest instantiated block
   // smallest instantiated block: 2 tiles (few slices of a narrow block: S = 4, b = 16 is 64 slice-columns).  Rounds 2-5 had the
   // two-matrix kernels from 4 (K2) / 3 (K3) tiles up only: the eigensolver's 4-slice passes on data whose missing calls take the dense
   // route multiplied 2 / 1 tiles of zero padding per launch (profiles/r06_missing_routes.txt)
   I8Shape sh{};
   sh.zb = (tiles + cap - 1) / cap;
   sh.nt = std::max(2, (tiles + sh.zb - 1) / sh.zb);
   // b = 16 with S = 7 slices: 112 slice-columns = 3.5 tiles -- the one-matrix kernel (the default route up to 0.5 % missing
   // calls) takes the remainder as a half tile
   // ... and so does b = 16 with S = 3 (48 slice-columns = 1.5 tiles: the eigensolver's cheap passes, one-matrix kernel only)
   sh.half = sh.zb == 1 && S * b == 32 * sh.nt - 16 && i8_rows4(two, mode, sh.nt, I8_HALF) != 0;
   // one matrix only (I8_NO_MISSING), both in a narrow column block, or a half tile: the accumulators fit a second row tile per wave
   // (64 rows x NT tiles)
   sh.rows = i8_rows4(two, mode, sh.nt, sh.half);
   sh.cols = 32 * sh.nt - (sh.half ? 16 : 0);
   sh.kc = 256;
   sh.wide = i8_exists(two, mode, sh.nt, sh.half, 512, I8_RM) || i8_exists(two, mode, sh.nt, sh.half, 512, I8_TL);
   return sh;
}

// Every shape gemm_i8 can be asked for has its instance -- same key, same tile -- in every layout gemm_i8 accepts for it, and at 512
// rows too where the shape says so
constexpr bool i8_shapes_have_instances()
{
   for (int S = 2; S <= 8; S++)
      for (int b = 16; b <= 64; b += 16)
         for (int two = 0; two < 2; two++)
            for (int mode = I8_FULL; mode <= I8_NO_MISSING; mode++) {
               if (two && mode == I8_NO_MISSING) continue;
               const I8Shape sh = i8_shape_static(S, b, two, mode);
               const auto has = [&](int rows, bool tiled) {
                  return i8_find(I8Instances{}, I8Key{two != 0, mode, sh.nt, sh.half, rows, tiled},
                                 [&](auto c) { return decltype(c)::COLS == sh.cols && decltype(c)::KC == sh.kc; });
               };
               for (int tiled = 0; tiled < 2; tiled++) {
                  if (tiled && !two && mode != I8_NO_MISSING) continue; // (gemm_i8 refuses it)
                  if (!has(sh.rows, tiled != 0) || (sh.wide && !has(512, tiled != 0))) return false;
               }
            }
   return true;
}
static_assert(i8_shapes_have_instances(), "a shape of i8_shape_static has no k_gemm_i8 instance: see I8Instances");

// rows_pad: the rows of the launch the shape is for (0: the 4-wave shape, whatever the launch)
static I8Shape i8_shape(int S, int b, bool two, int mode = I8_FULL, uint64_t rows_pad = 0)
{
   I8Shape sh = i8_shape_static(S, b, two, mode);
   if (rows_pad) sh.rows = i8_tile_rows(rows_pad, i8_ncu(), sh);
   return sh;
}

int gemm_i8_nsc_pad(int S, int b)
{
   const I8Shape s2 = i8_shape(S, b, false), s3 = i8_shape(S, b, true); // one padded width serves both kernels
   return std::max(s2.zb * 32 * s2.nt, s3.zb * 32 * s3.nt); // (whole tiles: the zero rows behind S*b carry zero weights)
}

// Work decomposition of one GEMM launch (see k_gemm_i8): one workgroup per CU (the 512-row tiles; two of the 256-row one-matrix
// tiles are co-resident, which the plan ignores -- its times are relative), so whole rounds of #CU tiles run unsplit
// (phase A) and only the leftover tiles are split along K (phase B); each extra split of phase B costs a partial plane
// for ITS rows only.  Plain split-K (nA = 0) is kept for problems with less than one round of tiles.
// (A stream-K schedule -- one persistent workgroup per CU walking a contiguous range of (tile, chunk) units -- was built
// and measured: it removes the round quantisation too, but it breaks the lock-step in which the workgroups of a round
// stream the same operand chunks through L2 and adds a prologue/epilogue per segment; net: K3 0.561 vs 0.568 ms at cfg2,
// +10 % time at cfg3.  Not kept.)
struct I8Plan {
   int nA, sB, cpsB;
   uint64_t rowB0, rowsB;
   unsigned grid;
};

static bool i8_verbose()
{
   static const bool verbose = FPCA_TEST_ENV("FPCA_I8_VERBOSE") != nullptr;
   return verbose;
}

static I8Plan i8_plan(uint64_t rows_pad, uint64_t k_pad, const I8Shape &sh, int bw)
{
   // force plain split-K with this factor (test builds), down to units of ONE chunk: a forced factor is not held to the four chunks per
   // split of the plan's own choices
   static const char *env_s = FPCA_TEST_ENV("FPCA_I8_SPLITS");
   const int forced = (env_s && atoi(env_s) > 0) ? std::min(atoi(env_s), 16) : 0;
   const int ncu = i8_ncu();
   const int rtiles = (int)((rows_pad + (sh.rows == 512 ? 511 : 0)) / sh.rows), rtl = (rtiles + 7) / 8, ids = 8 * rtl * sh.zb;
   const int chunks = (int)(k_pad / sh.kc);
   const double t_chunk = 2.2e-6 * (double)sh.rows * sh.cols * sh.kc / (128.0 * 256 * 256); // one workgroup-chunk at ~3 POP/s per CU: in proportion to the tile's rows
   const double t_seg = 5e-6;                                                               // prologue + epilogue of a workgroup
   const double t_row_plane = 2.0 * bw * 8 * 2 * sh.rows / 3.0e12;                          // one tile's partial, written + read
   double best = 1e30;
   int best_nA = 0, best_s = 1;
   const int nA_full = ids / ncu * ncu;
   for (int pass = 0; pass < 2; pass++) {
      const int nA = pass == 0 ? 0 : (nA_full == ids ? ids - ncu : nA_full);
      if (pass == 1 && (nA <= 0 || forced)) break;
      const int nB = ids - nA;
      for (int s = 1; s <= 16 && (s == 1 || (forced ? s <= chunks : s * 4 <= chunks)); s++) {
         if (pass == 0 && forced && s != std::min(forced, std::max(chunks, 1))) continue;
         const int cps = (chunks + s - 1) / s;
         const double tA = (double)(nA / ncu) * (chunks * t_chunk + t_seg);
         const double tB = (double)((nB * s + ncu - 1) / ncu) * (cps * t_chunk + t_seg);
         const double t = tA + tB + (s > 1 ? (double)s * nB * t_row_plane : 0.0);
         if (t < best * 0.995) {
            best = t;
            best_nA = nA;
            best_s = s;
         }
      }
   }
   I8Plan p;
   p.nA = best_nA;
   p.cpsB = (chunks + best_s - 1) / best_s;
   p.sB = (chunks + p.cpsB - 1) / p.cpsB; // no empty split
   const int qA = (p.nA / 8) / sh.zb;     // phase-B tiles have row tile >= 8 qA
   p.rowB0 = std::min<uint64_t>((uint64_t)qA * 8 * sh.rows, rows_pad);
   p.rowsB = rows_pad - p.rowB0;
   p.grid = (unsigned)(p.nA + (ids - p.nA) * p.sB);
   if (i8_verbose())
      std::fprintf(stderr, "[fpca] int8 GEMM plan: rows %llu K %llu tile %dx%d zb %d -> %d tile ids, %d chunks; %d unsplit + %d tiles x %d splits (%d chunks each), %u workgroups, est %.3f ms\n",
                   (unsigned long long)rows_pad, (unsigned long long)k_pad, sh.rows, sh.cols, sh.zb, ids, chunks, p.nA, ids - p.nA, p.sB, p.cpsB, p.grid,
                   best * 1e3);
   return p;
}

static int i8_bw(int b) // lcm(32, b) for b in {16, 32, 48, 64}
{
   return b == 48 ? 96 : std::max(b, 32);
}

// doubles of the workspace a plan uses: plane 0 of every row, planes 1 .. sB-1 of the phase-B rows
static size_t i8_plan_doubles(const I8Plan &p, uint64_t rows_pad, int zb, int bw)
{
   return ((size_t)rows_pad + (size_t)(p.sB - 1) * p.rowsB) * zb * 2 * (size_t)bw;
}

size_t gemm_i8_workspace_doubles(uint64_t rows_pad, uint64_t k_pad, int S, int b, bool two)
{
   size_t need = 0;
   for (int mode : {(int)I8_FULL, (int)I8_SKIP_EMPTY, (int)I8_NO_MISSING}) { // (the shapes differ: only FULL / NO_MISSING have the half tile)
      if (two && mode == I8_NO_MISSING) continue;
      const I8Shape sh = i8_shape(S, b, two, mode, rows_pad); // (the tile height gemm_i8 will choose for these rows)
      const I8Plan p = i8_plan(rows_pad, k_pad, sh, i8_bw(b));
      need = std::max(need, i8_plan_doubles(p, rows_pad, sh.zb, i8_bw(b)));
   }
   return need;
}

template <class C>
static void launch_i8(const I8Plan &pl, hipStream_t stream, const uint8_t *packed, size_t pitch, const int8_t *Qg, const int8_t *Qm,
                      uint64_t k_pad, const double *wg, const double *wm, int bw, double *ws, uint64_t rows_pad, int chunks_total, int zb, uint32_t tab1)
{
   static bool attr_set = false;
   if (!attr_set) {
      (void)hipFuncSetAttribute(reinterpret_cast<const void *>(&k_gemm_i8<C>), hipFuncAttributeMaxDynamicSharedMemorySize, C::LDS_BYTES);
      attr_set = true;
   }
   hipLaunchKernelGGL(HIP_KERNEL_NAME(k_gemm_i8<C>), dim3(pl.grid), dim3(C::THREADS), C::LDS_BYTES, stream, packed, pitch, Qg, Qm, k_pad, wg, wm, bw,
                      ws, rows_pad, chunks_total, zb, pl.nA, pl.sB, pl.cpsB, pl.rowB0, pl.rowsB, tab1);
}

CuFootprint gemm_i8_footprint(uint64_t rows_pad, int S, int b, bool two, int mode, bool e_only, bool tiled)
{
   const I8Shape sh = i8_shape(S, b, two, mode, rows_pad);
   const bool nt_p = i8_nt_p(I8Key{two, mode, sh.nt, sh.half, sh.rows, tiled}, e_only);
   CuFootprint f{0, 0, 0};
   i8_find(I8Instances{}, I8Key{two, mode, sh.nt, sh.half, sh.rows, tiled, nt_p}, [&](auto c) {
      using C = decltype(c);
      static int regs = 0; // (one per instance)
      if (!regs) {
         hipFuncAttributes attr;
         // unknown: as if a lane held half a SIMD's registers, which leaves a gather its one block per CU
         regs = hipFuncGetAttributes(&attr, reinterpret_cast<const void *>(&k_gemm_i8<C>)) == hipSuccess && attr.numRegs > 0 ? attr.numRegs : 256;
      }
      f = CuFootprint{C::WAVES, regs, C::LDS_BYTES};
      return true;
   });
   if (!f.waves) throw Error(-1, "gemm_i8: no kernel instance for this shape");
   return f;
}

void gemm_i8(const uint8_t *packed, size_t pitch, const int8_t *Qg, const int8_t *Qm, const double *wg, const double *wm,
             const long long *colsum_m, const double *mean, const double *sd, double *out, double *ws, uint64_t rows_pad, uint64_t k_pad,
             uint64_t rows_valid, int mode, const double *eplane /* I8_NO_MISSING kernel + E'Q computed elsewhere, or null */, int b,
             int S, const SliceOp *next_ops /* null, or the two operands whose column maxima the combine should leave */,
             hipStream_t stream, hipEvent_t *gemm_events /* null, or 2 events recorded around the GEMM kernel itself */,
             hipEvent_t before_combine /* null, or an event the combine must wait for (eplane produced on another stream) */,
             bool e_only /* mode 2 only: the missing-indicator matrix E alone, out = E Q (no statistics, no column sums) */,
             bool tiled /* `packed` is band-tiled: the two-matrix kernels and the G.M-alone ones have an instance for it */)
{
   const bool two = (Qg != Qm);
   if (tiled && !two && mode != I8_NO_MISSING) throw Error(-1, "gemm_i8: the one-operand kernels of both matrices read the row-major layout only");
   if (tiled && (pitch % 64 || k_pad > 4 * pitch)) throw Error(-1, "gemm_i8: a band-tiled copy has whole 64-byte chunks per row");
   if (e_only && (mode != I8_NO_MISSING || two)) throw Error(-1, "gemm_i8: e_only goes with the one-matrix kernel");
   const I8Shape sh = i8_shape(S, b, two, mode, rows_pad);
   const int bw = i8_bw(b); // Q holds gemm_i8_nsc_pad(S, b) rows; rows >= S*b are zero and carry zero weights
   const I8Plan pl = i8_plan(rows_pad, k_pad, sh, bw);
   const int chunks_total = (int)(k_pad / sh.kc);
   // (the plan line above is printed for the workspace sizing too: this one marks the plan that is launched, and the instance)
   const bool nt_p = i8_nt_p(I8Key{two, mode, sh.nt, sh.half, sh.rows, tiled}, e_only);
   if (i8_verbose())
      std::fprintf(stderr, "[fpca] int8 GEMM launch: %s, mode %d, nt %d%s, %s%s; phase B from row %llu; rows %d, loads %s\n", two ? "two operands" : "one operand", mode,
                   sh.nt, sh.half ? " (half tile)" : "", tiled ? "band-tiled" : "row-major", e_only ? ", E alone" : "", (unsigned long long)pl.rowB0,
                   sh.rows, nt_p ? "p" : "plain");
   // FPCA_DEBUG_I8_POISON (test builds): NaNs in exactly the extent of the workspace this plan uses -- plane 0 of every row, planes
   // 1 .. sB-1 of the phase-B rows -- so that a partial the kernel fails to write cannot pass for the previous launch's value
   static const bool poison = FPCA_TEST_ENV("FPCA_DEBUG_I8_POISON") != nullptr;
   if (poison) {
      const size_t used = i8_plan_doubles(pl, rows_pad, sh.zb, bw);
      if (hipMemsetAsync(ws, 0xFF, used * sizeof(double), stream) != hipSuccess) throw Error(-3, "gemm_i8: poisoning the workspace failed");
   }
   if (gemm_events) (void)hipEventRecord(gemm_events[0], stream);
   if (two && mode == I8_NO_MISSING) throw Error(-1, "gemm_i8: without missing genotypes both matrices share one operand (pass Qm == Qg)");
   // the instance of this shape at the tile height chosen for these rows, for the layout of `packed`: plan, kernel and combine then
   // walk the same tile grid
   const bool launched = i8_find(I8Instances{}, I8Key{two, mode, sh.nt, sh.half, sh.rows, tiled, nt_p}, [&](auto c) {
      using C = decltype(c);
      if (C::COLS != sh.cols || C::KC != sh.kc) throw Error(-1, "gemm_i8: the kernel instance and the shape disagree about the tile");
      launch_i8<C>(pl, stream, packed, pitch, Qg, Qm, k_pad, wg, wm, bw, ws, rows_pad, chunks_total, sh.zb, (e_only ? 0x00000100u : 0x00010002u));
      return true;
   });
   if (!launched) throw Error(-1, "gemm_i8: no kernel instance for this shape");
   launch_check();
   if (gemm_events) (void)hipEventRecord(gemm_events[1], stream);
   if (before_combine) (void)hipStreamWaitEvent(stream, before_combine, 0);
   const unsigned blocks = (unsigned)std::min<uint64_t>(1024, (rows_pad + (256 / b) - 1) / (256 / b));
   hipLaunchKernelGGL(k_i8_combine, dim3(blocks), dim3(256), 0, stream, ws, sh.zb, sh.rows, pl.nA, pl.sB, pl.rowB0, pl.rowsB, rows_pad, rows_valid, e_only ? -1 : mode == I8_NO_MISSING ? 1 : 2, eplane, b, bw, S, wm, colsum_m,
                      mean, sd, out,
                      next_ops ? next_ops[0].rowscale : nullptr, next_ops ? next_ops[0].maxbits : nullptr,
                      next_ops ? next_ops[1].rowscale : nullptr, next_ops ? next_ops[1].maxbits : nullptr);
   launch_check();
}

// per-SNP row scales of the K3 operands: inv_sd = 1/sd (0 for a monomorphic SNP, sd <= 1e-9, like the lookup table of
// data.cpp:300-320), mu_inv_sd = mean/sd
__global__ void k_i8_rowscales(const double *__restrict__ mean, const double *__restrict__ sd, uint64_t P_g, uint64_t P_pad,
                               double *__restrict__ inv_sd, double *__restrict__ mu_inv_sd)
{
   const uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x;
   if (j >= P_pad) return;
   double a = 0.0, m = 0.0;
   if (j < P_g && sd[j] > 1e-9) {
      a = 1.0 / sd[j];
      m = mean[j] / sd[j];
   }
   inv_sd[j] = a;
   mu_inv_sd[j] = m;
}

void i8_rowscales(const double *mean, const double *sd, uint64_t P_g, uint64_t P_pad, double *inv_sd, double *mu_inv_sd,
                  hipStream_t stream)
{
   hipLaunchKernelGGL(k_i8_rowscales, dim3((unsigned)((P_pad + 255) / 256)), dim3(256), 0, stream, mean, sd, P_g, P_pad, inv_sd, mu_inv_sd);
   launch_check();
}

// ------------------------------------------------------------------------------------------------
// sample-major copy of the packed stream for K3i: out[sample][snp/4] from in[snp][sample/4]  (2-bit transpose)
//   tile = 256 SNPs x 256 samples.  A thread loads the 16 x 16 block (16 SNP rows, one dword = 16 samples each; the 16
//   lanes of a sample-word run read 64 contiguous bytes of a row), transposes it in registers with the four
//   butterfly stages of a bit-matrix transpose on 2-bit elements, and the 256 blocks are regrouped through LDS so that
//   every thread stores 64 contiguous bytes (256 SNPs) of one sample row -- or, band-tiled (TILED, kernels.hpp
//   packed_piece_offset), the four 16-byte pieces of that (row, chunk): the workgroup's stores are eight whole 2 KB blocks.
template <bool TILED>
__global__ __launch_bounds__(256) void k_transpose_packed(const uint8_t *__restrict__ in, size_t pitch_in, uint8_t *__restrict__ out,
                                                           size_t pitch_out)
{
   __shared__ uint32_t tile[256][17];
   const uint64_t snp0 = (uint64_t)blockIdx.x * 256, smp0 = (uint64_t)blockIdx.y * 256;
   const int bs = threadIdx.x & 15, bp = threadIdx.x >> 4;
   uint32_t w[16];
#pragma unroll
   for (int i = 0; i < 16; i++) w[i] = *reinterpret_cast<const uint32_t *>(in + (snp0 + 16 * bp + i) * pitch_in + smp0 / 4 + 4 * bs);
   // w[i] holds (SNP i, samples 0..15); swap the off-diagonal sub-blocks at element distances 8, 4, 2, 1
#define FPCA_T2_STAGE(S_, MASK_)                                                    \
   _Pragma("unroll") for (int r = 0; r < 16; r++) if (!(r & S_))                    \
   {                                                                                \
      const uint32_t t = ((w[r] >> (2 * S_)) ^ w[r + S_]) & MASK_;                  \
      w[r + S_] ^= t;                                                               \
      w[r] ^= t << (2 * S_);                                                        \
   }
   FPCA_T2_STAGE(8, 0x0000FFFFu)
   FPCA_T2_STAGE(4, 0x00FF00FFu)
   FPCA_T2_STAGE(2, 0x0F0F0F0Fu)
   FPCA_T2_STAGE(1, 0x33333333u)
#undef FPCA_T2_STAGE
   // now w[j] holds (sample j, SNPs 0..15) of the block
#pragma unroll
   for (int j = 0; j < 16; j++) tile[16 * bs + j][bp] = w[j];
   __syncthreads();
   {
      const int r = threadIdx.x;
#pragma unroll
      for (int q = 0; q < 4; q++)
         *reinterpret_cast<u4 *>(out + packed_piece_offset(smp0 + r, snp0 / 64 + q, pitch_out, TILED)) =
            (u4){tile[r][4 * q], tile[r][4 * q + 1], tile[r][4 * q + 2], tile[r][4 * q + 3]};
   }
}

void transpose_packed(const uint8_t *in, size_t pitch_in, uint64_t N_pad, uint64_t P_pad, uint8_t *out, size_t pitch_out,
                      hipStream_t stream, bool tiled)
{
   if (N_pad % 256 || P_pad % 256) throw Error(-1, "transpose_packed: padded sizes must be multiples of 256");
   if (tiled && pitch_out % 64) throw Error(-1, "transpose_packed: a band-tiled copy has whole 64-byte chunks per row");
   dim3 grid((unsigned)(P_pad / 256), (unsigned)(N_pad / 256));
   if (tiled)
      hipLaunchKernelGGL(k_transpose_packed<true>, grid, dim3(256), 0, stream, in, pitch_in, out, pitch_out);
   else
      hipLaunchKernelGGL(k_transpose_packed<false>, grid, dim3(256), 0, stream, in, pitch_in, out, pitch_out);
   launch_check();
}

// the band-tiled arrangement of row-major records (the copy K2 streams): a thread moves the four 16-byte pieces of one (row, chunk);
// a wave reads 64 B of 64 rows and writes two whole 2 KB blocks
__global__ __launch_bounds__(256) void k_tile_packed(const uint8_t *__restrict__ in, size_t pitch, uint8_t *__restrict__ out)
{
   const uint64_t r = (uint64_t)blockIdx.y * 256 + threadIdx.x, c = blockIdx.x;
   u4 v[4];
#pragma unroll
   for (int q = 0; q < 4; q++) v[q] = *reinterpret_cast<const u4 *>(in + packed_piece_offset(r, 4 * c + q, pitch, false));
#pragma unroll
   for (int q = 0; q < 4; q++) *reinterpret_cast<u4 *>(out + packed_piece_offset(r, 4 * c + q, pitch, true)) = v[q];
}

void tile_packed(const uint8_t *in, size_t pitch, uint64_t rows, uint8_t *out, hipStream_t stream)
{
   if (rows % 256 || pitch % 64) throw Error(-1, "tile_packed: rows in multiples of 256, whole 64-byte chunks per row");
   if (!rows) return;
   hipLaunchKernelGGL(k_tile_packed, dim3((unsigned)(pitch / 64), (unsigned)(rows / 256)), dim3(256), 0, stream, in, pitch, out);
   launch_check();
}

// diagnostic: C(32x32) = A(32x32 int8) * B(32x32 int8)^T-style product through v_mfma_i32_32x32x32_i8 with the operand
// mapping used above: lane l supplies 16 bytes of A row l&31 and of B column l&31 for k = 16 (l>>5) .. +15
__global__ void k_mfma_i8_probe(const int8_t *A /*[32][32] row-major: A[i][k]*/, const int8_t *Bt /*[32][32]: Bt[j][k]*/, int *D)
{
   const int lane = threadIdx.x & 63, li = lane & 31, kh = lane >> 5;
   v4i a = *reinterpret_cast<const v4i *>(A + li * 32 + kh * 16);
   v4i b = *reinterpret_cast<const v4i *>(Bt + li * 32 + kh * 16);
   v16i acc;
   for (int r = 0; r < 16; r++) acc[r] = 0;
   acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(a, b, acc, 0, 0, 0);
   for (int r = 0; r < 16; r++) D[((r & 3) + 8 * (r >> 2) + 4 * kh) * 32 + li] = acc[r];
}

void mfma_i8_probe(const int8_t *A, const int8_t *Bt, int *D, hipStream_t stream)
{
   hipLaunchKernelGGL(k_mfma_i8_probe, dim3(1), dim3(64), 0, stream, A, Bt, D);
   launch_check();
}

// diagnostic: the two int8 instructions of k_gemm_i8 with their operands in the given order or EXCHANGED, stored through the register
// map of the given order -- exchanged, the same registers hold the transposed tile.
//   shape 32: v_mfma_i32_32x32x32_i8, A[32][32], Bt[32][32], D[32][32]      (k_mfma_i8_probe's layout)
//   shape 16: v_mfma_i32_16x16x64_i8, A[16][64], Bt[16][64], D[16][16]: lane l supplies bytes 16 (l >> 4) .. of row / column l & 15;
//             register r of lane l = D[4 (l >> 4) + r][l & 15]
__global__ void k_mfma_i8_ports(int shape, int exchanged, const int8_t *A, const int8_t *Bt, int *D)
{
   const int lane = threadIdx.x & 63;
   if (shape == 32) {
      const int li = lane & 31, kh = lane >> 5;
      const v4i a = *reinterpret_cast<const v4i *>(A + li * 32 + kh * 16), b = *reinterpret_cast<const v4i *>(Bt + li * 32 + kh * 16);
      v16i acc;
      for (int r = 0; r < 16; r++) acc[r] = 0;
      acc = exchanged ? __builtin_amdgcn_mfma_i32_32x32x32_i8(b, a, acc, 0, 0, 0) : __builtin_amdgcn_mfma_i32_32x32x32_i8(a, b, acc, 0, 0, 0);
      for (int r = 0; r < 16; r++) D[((r & 3) + 8 * (r >> 2) + 4 * kh) * 32 + li] = acc[r];
   } else {
      const int lj = lane & 15, qd = lane >> 4;
      const v4i a = *reinterpret_cast<const v4i *>(A + lj * 64 + qd * 16), b = *reinterpret_cast<const v4i *>(Bt + lj * 64 + qd * 16);
      v4i acc = {0, 0, 0, 0};
      acc = exchanged ? __builtin_amdgcn_mfma_i32_16x16x64_i8(b, a, acc, 0, 0, 0) : __builtin_amdgcn_mfma_i32_16x16x64_i8(a, b, acc, 0, 0, 0);
      for (int r = 0; r < 4; r++) D[(4 * qd + r) * 16 + lj] = acc[r];
   }
}

void mfma_i8_ports(int shape, bool exchanged, const int8_t *A, const int8_t *Bt, int *D, hipStream_t stream)
{
   hipLaunchKernelGGL(k_mfma_i8_ports, dim3(1), dim3(64), 0, stream, shape, exchanged ? 1 : 0, A, Bt, D);
   launch_check();
}

// issue-rate ceiling of v_mfma_i32_32x32x32_i8: 8 independent accumulators per wave, explicit registers (the compiler
// must not reorder or shuffle them).  The rate is power-limited, so what the operands hold and how often they change matters: each
// port has two register sets (A: v128-131 / v132-135, B: v136-139 / v140-143), each filled by its own kind and seed (I8PeakFill).
//   order 0: A alternates its sets every instruction, B holds one set for two   (A0 B0, A1 B0, A0 B1, A1 B1)
//   order 1: A holds one set for two instructions, B alternates every one       (A0 B0, A0 B1, A1 B0, A1 B1)
// (with equal sets nothing changes between instructions and the order is immaterial)
#define I8_PEAK_CLOBBERS "v0", "v1", "v2", "v3", "v4", "v5", "v6", "v7", "v8", "v9", "v10", "v11", "v12", "v13", "v14", "v15", "v16", "v17", "v18", "v19", "v20", "v21", "v22", "v23", "v24", "v25", "v26", "v27", "v28", "v29", "v30", "v31", "v32", "v33", "v34", "v35", "v36", "v37", "v38", "v39", "v40", "v41", "v42", "v43", "v44", "v45", "v46", "v47", "v48", "v49", "v50", "v51", "v52", "v53", "v54", "v55", "v56", "v57", "v58", "v59", "v60", "v61", "v62", "v63", "v64", "v65", "v66", "v67", "v68", "v69", "v70", "v71", "v72", "v73", "v74", "v75", "v76", "v77", "v78", "v79", "v80", "v81", "v82", "v83", "v84", "v85", "v86", "v87", "v88", "v89", "v90", "v91", "v92", "v93", "v94", "v95", "v96", "v97", "v98", "v99", "v100", "v101", "v102", "v103", "v104", "v105", "v106", "v107", "v108", "v109", "v110", "v111", "v112", "v113", "v114", "v115", "v116", "v117", "v118", "v119", "v120", "v121", "v122", "v123", "v124", "v125", "v126", "v127", "v128", "v129", "v130", "v131", "v132", "v133", "v134", "v135", "v136", "v137", "v138", "v139", "v140", "v141", "v142", "v143"
__global__ __launch_bounds__(256, 1) void k_mfma_i8_peak(int *out, int iters, I8PeakFill fl)
{
   const uint32_t l = threadIdx.x * 2654435761u;
   uint32_t f[4][4]; // [A set 0, A set 1, B set 0, B set 1][dword]
#pragma unroll
   for (int s = 0; s < 4; s++) {
      const uint32_t kind = fl.kind[s];
      uint32_t h[4];
      h[0] = (fl.seed[s] ^ l) * 0x9E3779B1u;
      h[1] = (h[0] >> 3) * 0x85EBCA6Bu;
      h[2] = (h[1] >> 5) * 0xC2B2AE35u;
      h[3] = (h[2] >> 7) * 0x27D4EB2Fu;
#pragma unroll
      for (int q = 0; q < 4; q++) {
         uint32_t g = 0; // I8_FILL_GENO: every hashed byte x becomes 3 x >> 8, a third each of 0, 1 and 2
#pragma unroll
         for (int k = 0; k < 4; k++) g |= ((((h[q] >> (8 * k)) & 0xffu) * 3u) >> 8) << (8 * k);
         f[s][q] = kind == I8_FILL_ZERO ? 0u : kind == I8_FILL_GENO ? g : h[q];
      }
   }
   asm volatile(
      "v_mov_b32 v0, 0\n\t"
      "v_mov_b32 v1, 0\n\t"
      "v_mov_b32 v2, 0\n\t"
      "v_mov_b32 v3, 0\n\t"
      "v_mov_b32 v4, 0\n\t"
      "v_mov_b32 v5, 0\n\t"
      "v_mov_b32 v6, 0\n\t"
      "v_mov_b32 v7, 0\n\t"
      "v_mov_b32 v8, 0\n\t"
      "v_mov_b32 v9, 0\n\t"
      "v_mov_b32 v10, 0\n\t"
      "v_mov_b32 v11, 0\n\t"
      "v_mov_b32 v12, 0\n\t"
      "v_mov_b32 v13, 0\n\t"
      "v_mov_b32 v14, 0\n\t"
      "v_mov_b32 v15, 0\n\t"
      "v_mov_b32 v16, 0\n\t"
      "v_mov_b32 v17, 0\n\t"
      "v_mov_b32 v18, 0\n\t"
      "v_mov_b32 v19, 0\n\t"
      "v_mov_b32 v20, 0\n\t"
      "v_mov_b32 v21, 0\n\t"
      "v_mov_b32 v22, 0\n\t"
      "v_mov_b32 v23, 0\n\t"
      "v_mov_b32 v24, 0\n\t"
      "v_mov_b32 v25, 0\n\t"
      "v_mov_b32 v26, 0\n\t"
      "v_mov_b32 v27, 0\n\t"
      "v_mov_b32 v28, 0\n\t"
      "v_mov_b32 v29, 0\n\t"
      "v_mov_b32 v30, 0\n\t"
      "v_mov_b32 v31, 0\n\t"
      "v_mov_b32 v32, 0\n\t"
      "v_mov_b32 v33, 0\n\t"
      "v_mov_b32 v34, 0\n\t"
      "v_mov_b32 v35, 0\n\t"
      "v_mov_b32 v36, 0\n\t"
      "v_mov_b32 v37, 0\n\t"
      "v_mov_b32 v38, 0\n\t"
      "v_mov_b32 v39, 0\n\t"
      "v_mov_b32 v40, 0\n\t"
      "v_mov_b32 v41, 0\n\t"
      "v_mov_b32 v42, 0\n\t"
      "v_mov_b32 v43, 0\n\t"
      "v_mov_b32 v44, 0\n\t"
      "v_mov_b32 v45, 0\n\t"
      "v_mov_b32 v46, 0\n\t"
      "v_mov_b32 v47, 0\n\t"
      "v_mov_b32 v48, 0\n\t"
      "v_mov_b32 v49, 0\n\t"
      "v_mov_b32 v50, 0\n\t"
      "v_mov_b32 v51, 0\n\t"
      "v_mov_b32 v52, 0\n\t"
      "v_mov_b32 v53, 0\n\t"
      "v_mov_b32 v54, 0\n\t"
      "v_mov_b32 v55, 0\n\t"
      "v_mov_b32 v56, 0\n\t"
      "v_mov_b32 v57, 0\n\t"
      "v_mov_b32 v58, 0\n\t"
      "v_mov_b32 v59, 0\n\t"
      "v_mov_b32 v60, 0\n\t"
      "v_mov_b32 v61, 0\n\t"
      "v_mov_b32 v62, 0\n\t"
      "v_mov_b32 v63, 0\n\t"
      "v_mov_b32 v64, 0\n\t"
      "v_mov_b32 v65, 0\n\t"
      "v_mov_b32 v66, 0\n\t"
      "v_mov_b32 v67, 0\n\t"
      "v_mov_b32 v68, 0\n\t"
      "v_mov_b32 v69, 0\n\t"
      "v_mov_b32 v70, 0\n\t"
      "v_mov_b32 v71, 0\n\t"
      "v_mov_b32 v72, 0\n\t"
      "v_mov_b32 v73, 0\n\t"
      "v_mov_b32 v74, 0\n\t"
      "v_mov_b32 v75, 0\n\t"
      "v_mov_b32 v76, 0\n\t"
      "v_mov_b32 v77, 0\n\t"
      "v_mov_b32 v78, 0\n\t"
      "v_mov_b32 v79, 0\n\t"
      "v_mov_b32 v80, 0\n\t"
      "v_mov_b32 v81, 0\n\t"
      "v_mov_b32 v82, 0\n\t"
      "v_mov_b32 v83, 0\n\t"
      "v_mov_b32 v84, 0\n\t"
      "v_mov_b32 v85, 0\n\t"
      "v_mov_b32 v86, 0\n\t"
      "v_mov_b32 v87, 0\n\t"
      "v_mov_b32 v88, 0\n\t"
      "v_mov_b32 v89, 0\n\t"
      "v_mov_b32 v90, 0\n\t"
      "v_mov_b32 v91, 0\n\t"
      "v_mov_b32 v92, 0\n\t"
      "v_mov_b32 v93, 0\n\t"
      "v_mov_b32 v94, 0\n\t"
      "v_mov_b32 v95, 0\n\t"
      "v_mov_b32 v96, 0\n\t"
      "v_mov_b32 v97, 0\n\t"
      "v_mov_b32 v98, 0\n\t"
      "v_mov_b32 v99, 0\n\t"
      "v_mov_b32 v100, 0\n\t"
      "v_mov_b32 v101, 0\n\t"
      "v_mov_b32 v102, 0\n\t"
      "v_mov_b32 v103, 0\n\t"
      "v_mov_b32 v104, 0\n\t"
      "v_mov_b32 v105, 0\n\t"
      "v_mov_b32 v106, 0\n\t"
      "v_mov_b32 v107, 0\n\t"
      "v_mov_b32 v108, 0\n\t"
      "v_mov_b32 v109, 0\n\t"
      "v_mov_b32 v110, 0\n\t"
      "v_mov_b32 v111, 0\n\t"
      "v_mov_b32 v112, 0\n\t"
      "v_mov_b32 v113, 0\n\t"
      "v_mov_b32 v114, 0\n\t"
      "v_mov_b32 v115, 0\n\t"
      "v_mov_b32 v116, 0\n\t"
      "v_mov_b32 v117, 0\n\t"
      "v_mov_b32 v118, 0\n\t"
      "v_mov_b32 v119, 0\n\t"
      "v_mov_b32 v120, 0\n\t"
      "v_mov_b32 v121, 0\n\t"
      "v_mov_b32 v122, 0\n\t"
      "v_mov_b32 v123, 0\n\t"
      "v_mov_b32 v124, 0\n\t"
      "v_mov_b32 v125, 0\n\t"
      "v_mov_b32 v126, 0\n\t"
      "v_mov_b32 v127, 0\n\t"
      ::: I8_PEAK_CLOBBERS);
   asm volatile(
      "v_mov_b32 v128, %0\n\t"
      "v_mov_b32 v129, %1\n\t"
      "v_mov_b32 v130, %2\n\t"
      "v_mov_b32 v131, %3\n\t"
      "v_mov_b32 v132, %4\n\t"
      "v_mov_b32 v133, %5\n\t"
      "v_mov_b32 v134, %6\n\t"
      "v_mov_b32 v135, %7\n\t"
      "v_mov_b32 v136, %8\n\t"
      "v_mov_b32 v137, %9\n\t"
      "v_mov_b32 v138, %10\n\t"
      "v_mov_b32 v139, %11\n\t"
      "v_mov_b32 v140, %12\n\t"
      "v_mov_b32 v141, %13\n\t"
      "v_mov_b32 v142, %14\n\t"
      "v_mov_b32 v143, %15\n\t"
      :: "v"(f[0][0]), "v"(f[0][1]), "v"(f[0][2]), "v"(f[0][3]), "v"(f[1][0]), "v"(f[1][1]), "v"(f[1][2]), "v"(f[1][3]), "v"(f[2][0]), "v"(f[2][1]), "v"(f[2][2]), "v"(f[2][3]), "v"(f[3][0]), "v"(f[3][1]), "v"(f[3][2]), "v"(f[3][3]) : I8_PEAK_CLOBBERS);
   if (fl.order == 0)
      for (int it = 0; it < iters; it++) {
         asm volatile(
            "v_mfma_i32_32x32x32_i8 v[0:15], v[128:131], v[136:139], v[0:15]\n\t"
            "v_mfma_i32_32x32x32_i8 v[16:31], v[132:135], v[136:139], v[16:31]\n\t"
            "v_mfma_i32_32x32x32_i8 v[32:47], v[128:131], v[140:143], v[32:47]\n\t"
            "v_mfma_i32_32x32x32_i8 v[48:63], v[132:135], v[140:143], v[48:63]\n\t"
            "v_mfma_i32_32x32x32_i8 v[64:79], v[128:131], v[136:139], v[64:79]\n\t"
            "v_mfma_i32_32x32x32_i8 v[80:95], v[132:135], v[136:139], v[80:95]\n\t"
            "v_mfma_i32_32x32x32_i8 v[96:111], v[128:131], v[140:143], v[96:111]\n\t"
            "v_mfma_i32_32x32x32_i8 v[112:127], v[132:135], v[140:143], v[112:127]\n\t"
            ::: I8_PEAK_CLOBBERS);
      }
   else
      for (int it = 0; it < iters; it++) {
         asm volatile(
            "v_mfma_i32_32x32x32_i8 v[0:15], v[128:131], v[136:139], v[0:15]\n\t"
            "v_mfma_i32_32x32x32_i8 v[16:31], v[128:131], v[140:143], v[16:31]\n\t"
            "v_mfma_i32_32x32x32_i8 v[32:47], v[132:135], v[136:139], v[32:47]\n\t"
            "v_mfma_i32_32x32x32_i8 v[48:63], v[132:135], v[140:143], v[48:63]\n\t"
            "v_mfma_i32_32x32x32_i8 v[64:79], v[128:131], v[136:139], v[64:79]\n\t"
            "v_mfma_i32_32x32x32_i8 v[80:95], v[128:131], v[140:143], v[80:95]\n\t"
            "v_mfma_i32_32x32x32_i8 v[96:111], v[132:135], v[136:139], v[96:111]\n\t"
            "v_mfma_i32_32x32x32_i8 v[112:127], v[132:135], v[140:143], v[112:127]\n\t"
            ::: I8_PEAK_CLOBBERS);
      }
   int r;
   asm volatile("s_nop 7\n\ts_nop 7\n\tv_mov_b32 %0, v0" : "=v"(r)::I8_PEAK_CLOBBERS);
   if (r == 0x7fffffff) out[threadIdx.x] = r;
}
#undef I8_PEAK_CLOBBERS

double mfma_i8_peak_tops(int waves_per_simd, int iters, const I8PeakFill &fill, hipStream_t stream)
{
   DevMem<int> d(1024, "fpca_debug_mfma_peak", "the probe's output words");
   const int blocks = 256 * waves_per_simd;
   DevEvent e0("fpca_debug_mfma_peak"), e1("fpca_debug_mfma_peak");
   hipLaunchKernelGGL(k_mfma_i8_peak, dim3(blocks), dim3(256), 0, stream, d.p, iters / 10, fill);
   (void)hipEventRecord(e0, stream);
   hipLaunchKernelGGL(k_mfma_i8_peak, dim3(blocks), dim3(256), 0, stream, d.p, iters, fill);
   (void)hipEventRecord(e1, stream);
   (void)hipEventSynchronize(e1);
   const float ms = elapsed_ms(e0, e1);
   const double ops = (double)blocks * 4 /*waves*/ * (double)iters * 8 * 65536.0;
   return ops / (ms * 1e-3) / 1e12;
}

} // namespace kern
} // namespace fpca
