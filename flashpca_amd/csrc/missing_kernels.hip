// missing_kernels.hip -- the missing-call side of the exact-integer mode: index lists of the missing calls of the 2-bit records, the
// gather-sums over them (the sparse missing-indicator route) and the row shuffles of the hybrid route.  Callers: missing_routes.hip
// and the debug hooks; the int8 GEMM these routes feed is kernels_i8.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <mutex>

#include "common.hpp"
#include "kernels.hpp"
#include "launch_check.hpp"

namespace fpca {
namespace kern {

typedef uint32_t u4 __attribute__((ext_vector_type(4)));

// ------------------------------------------------------------------------------------------------
// Sparse missing indicator.  With a typical array-data missing rate (0.1 %) the E half of the int8 work multiplies a
// matrix that is 99.9 % zeros.  Instead: index lists of the missing calls (per SNP for K2, per sample for K3), built
// once, and  E'B  /  E (mean T / sd)  as gathers of fp64 rows -- 256 bytes per missing call, a few ms where the MFMA
// route took 8-9 -- while the int8 GEMM multiplies G.M alone with the one-matrix kernel.

// missing calls of each 2-bit record among its first `ncols` codes
// (tiled: the records are in the band-tiled layout -- byte j of a record sits in its 16-byte piece j / 16)
__global__ __launch_bounds__(256) void k_count_missing(const uint8_t *__restrict__ packed, size_t pitch, uint64_t ncols,
                                                        uint32_t *__restrict__ cnt, bool tiled)
{
   const uint64_t rec = blockIdx.x;
   auto byte_at = [&](uint64_t j) { return packed + packed_piece_offset(rec, j >> 4, pitch, tiled) + (j & 15); };
   const uint64_t nbytes = (ncols + 3) / 4, nw = nbytes / 4;
   uint32_t n = 0;
   for (uint64_t i = threadIdx.x; i < nw; i += 256) {
      const uint32_t w = *reinterpret_cast<const uint32_t *>(byte_at(4 * i));
      n += __popc(w & ~(w >> 1) & 0x55555555u);
   }
   for (uint64_t i = nw * 4 + threadIdx.x; i < nbytes; i += 256) {
      const uint32_t w = *byte_at(i);
      n += __popc(w & ~(w >> 1) & 0x55u);
   }
   // codes beyond ncols in the last byte
   if (threadIdx.x == 0 && (ncols & 3)) {
      const uint32_t w = *byte_at(nbytes - 1) >> (2 * (ncols & 3));
      n -= __popc(w & ~(w >> 1) & 0x55u);
   }
   __shared__ uint32_t red[256];
   red[threadIdx.x] = n;
   __syncthreads();
   for (int o = 128; o > 0; o >>= 1) {
      if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
      __syncthreads();
   }
   if (threadIdx.x == 0) cnt[blockIdx.x] = red[0];
}

// idx[ptr[r] ..] = ascending positions (< ncols) of the missing calls of record r.  The record is walked in tiles of 1024
// dwords (coalesced 16-byte loads), every thread owns four consecutive dwords = 64 codes; a wave scan + 4 wave totals
// place each thread's hits.  (Rows are 128-byte aligned and padded with "missing" codes up to the pitch, so whole
// 16-byte pieces can be read; positions >= ncols are masked off.)
__global__ __launch_bounds__(256) void k_fill_missing(const uint8_t *__restrict__ packed, size_t pitch, uint64_t ncols,
                                                       const uint32_t *__restrict__ ptr, uint32_t *__restrict__ idx, bool tiled)
{
   const uint64_t nq = (ncols + 63) / 64; // 16-byte pieces holding valid codes
   const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
   __shared__ uint32_t wsum[4];
   uint32_t base = ptr[blockIdx.x];
   if (ptr[blockIdx.x + 1] == base) return; // nothing to list: a record without a missing call -- or one whose missing calls go the
                                            // dense route (its count was set to zero on purpose, missing_routes.hip ensure_hybrid)
   for (uint64_t q0 = 0; q0 < nq; q0 += 256) {
      const uint64_t q = q0 + threadIdx.x;
      uint32_t m[4] = {0u, 0u, 0u, 0u};
      if (q < nq) {
         const u4 x = *reinterpret_cast<const u4 *>(packed + packed_piece_offset(blockIdx.x, q, pitch, tiled));
#pragma unroll
         for (int k = 0; k < 4; k++) {
            m[k] = x[k] & ~(x[k] >> 1) & 0x55555555u;
            const uint64_t first = q * 64 + 16 * k; // first code of this dword
            if (first >= ncols)
               m[k] = 0u;
            else if (ncols - first < 16)
               m[k] &= (1u << (2 * (ncols - first))) - 1u;
         }
      }
      const uint32_t c = __popc(m[0]) + __popc(m[1]) + __popc(m[2]) + __popc(m[3]);
      uint32_t v = c;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
         const uint32_t t = __shfl_up(v, o);
         if (lane >= o) v += t;
      }
      if (lane == 63) wsum[wave] = v;
      __syncthreads();
      uint32_t woff = 0, total = 0;
#pragma unroll
      for (int k = 0; k < 4; k++) {
         if (k < wave) woff += wsum[k];
         total += wsum[k];
      }
      uint32_t pos = base + woff + v - c;
#pragma unroll
      for (int k = 0; k < 4; k++) {
         uint32_t mk = m[k];
         while (mk) {
            const int bit = __ffs(mk) - 1;
            idx[pos++] = (uint32_t)(q * 64 + 16 * k + bit / 2);
            mk &= mk - 1;
         }
      }
      base += total;
      __syncthreads();
   }
}

void count_missing(const uint8_t *packed, size_t pitch, uint64_t ncols, uint64_t nrec, uint32_t *cnt, hipStream_t stream, bool tiled)
{
   if (!nrec) return;
   hipLaunchKernelGGL(k_count_missing, dim3((unsigned)nrec), dim3(256), 0, stream, packed, pitch, ncols, cnt, tiled);
   launch_check();
}

void fill_missing(const uint8_t *packed, size_t pitch, uint64_t ncols, uint64_t nrec, const uint32_t *ptr, uint32_t *idx, hipStream_t stream,
                  bool tiled)
{
   if (!nrec) return;
   hipLaunchKernelGGL(k_fill_missing, dim3((unsigned)nrec), dim3(256), 0, stream, packed, pitch, ncols, ptr, idx, tiled);
   launch_check();
}

// two adjacent columns of a row, fetched by one load (16 bytes of an fp64 row, 8 of an fp32 one)
template <class VT>
struct ColPair;
template <>
struct ColPair<double> {
   typedef double2 type;
};
template <>
struct ColPair<float> {
   typedef float2 type;
};

// out[r][c] = sum over s in list(r) of V[s][c] * (rowscale ? rowscale[s] : 1)   (fp64, list order = ascending s);
// rows r >= nrec are zeroed.  One wave per output row.  A lane holds two adjacent columns, B / 2 lanes a row: 2 EPW = 128 / b list
// entries per step, 2 steps in flight.  The sums are those of one column per lane with EPW entries per step and 4 steps in flight,
// bit for bit: entry n of a list goes to partial sum n mod 4 EPW, which is accumulator (n / 2 EPW) mod 2 of lane group n mod 2 EPW
// here and was accumulator (n / EPW) mod 4 of lane group n mod EPW there; the partial sums of a column are then added in the order
// (a0 + a1) + (a2 + a3) per old lane group -- a0, a2 from lane group g, a1, a3 from lane group g + EPW, 32 lanes up -- and across
// the old lane groups by the same tree.
template <int B, class VT>
__global__ __launch_bounds__(256) void k_sparse_rows_sum(const uint32_t *__restrict__ ptr, const uint32_t *__restrict__ idx,
                                                          const VT *__restrict__ V, const double *__restrict__ rowscale, uint64_t nrec,
                                                          uint64_t rows_out, double *__restrict__ out, const double *__restrict__ init,
                                                          const double *__restrict__ colw)
{
   typedef typename ColPair<VT>::type V2;
   constexpr int EPW = 64 / B, LPR = B / 2, G2 = 2 * EPW;
   const int lane = threadIdx.x & 63, c2 = lane % LPR, e0 = lane / LPR;
   const V2 *__restrict__ V2p = reinterpret_cast<const V2 *>(V);
   for (uint64_t r = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6); r < rows_out; r += (uint64_t)gridDim.x * 4) {
      double a0x = 0.0, a0y = 0.0, a1x = 0.0, a1y = 0.0;
      if (r < nrec) {
         const uint32_t p0 = ptr[r], p1 = ptr[r + 1];
         for (uint32_t t = p0 + e0; t < p1; t += 2 * G2) {
            const uint32_t t1 = t + G2;
            const uint32_t s0 = idx[t], s1 = t1 < p1 ? idx[t1] : 0;
            const V2 w0 = V2p[(uint64_t)s0 * LPR + c2];
            double v0x = w0.x, v0y = w0.y, v1x = 0.0, v1y = 0.0;
            if (t1 < p1) {
               const V2 w1 = V2p[(uint64_t)s1 * LPR + c2];
               v1x = w1.x;
               v1y = w1.y;
            }
            if (rowscale) {
               const double f0 = rowscale[s0], f1 = t1 < p1 ? rowscale[s1] : 0.0;
               v0x *= f0;
               v0y *= f0;
               v1x *= f1;
               v1y *= f1;
            }
            a0x += v0x;
            a0y += v0y;
            a1x += v1x;
            a1y += v1y;
         }
      }
      a0x += __shfl_down(a0x, 32);
      a0y += __shfl_down(a0y, 32);
      a1x += __shfl_down(a1x, 32);
      a1y += __shfl_down(a1y, 32);
      double ax = a0x + a1x, ay = a0y + a1y;
#pragma unroll
      for (int o = 16; o >= LPR; o >>= 1) {
         ax += __shfl_down(ax, o);
         ay += __shfl_down(ay, o);
      }
      if (lane < LPR) {
         const int c = 2 * c2;
         if (colw) { // fp32 rows were stored as x 2^(1 - e_c); colw[c] = 2^(e_c - 6) (top slice's weight)
            ax *= colw[c] * 32.0;
            ay *= colw[c + 1] * 32.0;
         }
         out[r * B + c] = init ? init[r * B + c] + ax : ax;
         out[r * B + c + 1] = init ? init[r * B + c + 1] + ay : ay;
      }
   }
}

// The same sum with the index list read in coalesced batches of 64 (one entry per lane, broadcast by shuffles) instead of
// one dependent 4-byte load per gathered row: the loop above is a chain idx -> row of V, both at Infinity-Cache latency,
// with two row pieces in flight per lane; here the rows of a batch are independent of any further index load and four pieces
// are in flight (per lane slot).  The per-row factors of a batch are gathered once, one per lane, the same way.
// (Two columns per lane as above: partial sum n mod 8 EPW of a column is accumulator (n / 2 EPW) mod 4 of lane group n mod 2 EPW,
// was accumulator (n / EPW) mod 8 of lane group n mod EPW, and the additions keep their order.)
template <int B, class VT>
__global__ __launch_bounds__(256) void k_sparse_rows_sum_batched(const uint32_t *__restrict__ ptr, const uint32_t *__restrict__ idx,
                                                                  const VT *__restrict__ V, const double *__restrict__ rowscale,
                                                                  uint64_t nrec, uint64_t rows_out, double *__restrict__ out, const double *__restrict__ init,
                                                                  const double *__restrict__ colw)
{
   typedef typename ColPair<VT>::type V2;
   constexpr int EPW = 64 / B, LPR = B / 2, G2 = 2 * EPW, U = 4;
   const int lane = threadIdx.x & 63, c2 = lane % LPR, e0 = lane / LPR;
   const V2 *__restrict__ V2p = reinterpret_cast<const V2 *>(V);
   for (uint64_t r = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6); r < rows_out; r += (uint64_t)gridDim.x * 4) {
      double accx[U], accy[U];
#pragma unroll
      for (int u = 0; u < U; u++) accx[u] = accy[u] = 0.0;
      if (r < nrec) {
         const uint32_t p0 = ptr[r], p1 = ptr[r + 1];
         for (uint32_t t0 = p0; t0 < p1; t0 += 64) {
            const int cnt = (int)(p1 - t0 < 64u ? p1 - t0 : 64u);
            const uint32_t mine = lane < cnt ? idx[t0 + lane] : 0u;
            const double myscale = (rowscale && lane < cnt) ? rowscale[mine] : 1.0;
            for (int u0 = 0; u0 < cnt; u0 += G2 * U) {
#pragma unroll
               for (int u = 0; u < U; u++) {
                  const int e = u0 + u * G2 + e0;
                  const uint32_t srow = (uint32_t)__shfl((int)mine, e & 63);
                  const double sc = __shfl(myscale, e & 63);
                  if (e < cnt) {
                     const V2 w = V2p[(uint64_t)srow * LPR + c2];
                     accx[u] += w.x * sc;
                     accy[u] += w.y * sc;
                  }
               }
            }
         }
      }
#pragma unroll
      for (int u = 0; u < U; u++) {
         accx[u] += __shfl_down(accx[u], 32);
         accy[u] += __shfl_down(accy[u], 32);
      }
      double ax = (accx[0] + accx[1]) + (accx[2] + accx[3]), ay = (accy[0] + accy[1]) + (accy[2] + accy[3]);
#pragma unroll
      for (int o = 16; o >= LPR; o >>= 1) {
         ax += __shfl_down(ax, o);
         ay += __shfl_down(ay, o);
      }
      if (lane < LPR) {
         const int c = 2 * c2;
         if (colw) { // fp32 rows were stored as x 2^(1 - e_c); colw[c] = 2^(e_c - 6) (top slice's weight)
            ax *= colw[c] * 32.0;
            ay *= colw[c + 1] * 32.0;
         }
         out[r * B + c] = init ? init[r * B + c] + ax : ax;
         out[r * B + c + 1] = init ? init[r * B + c + 1] + ay : ay;
      }
   }
}

// Short lists (a dozen entries per row: the samples of a 1/8 SNP shard, small problems): with one wave per row the chain
// ptr -> idx -> rows is three dependent round trips per row and nothing else in flight in that wave -- latency-bound (4 TB/s
// out of an L2-resident operand).  Here 64 / B rows share a wave, B lanes (one per column) each, every group walking its own
// list four entries at a time: four times the rows in flight, no cross-lane reduction.
template <int B, class VT>
__global__ __launch_bounds__(256) void k_sparse_rows_sum_short(const uint32_t *__restrict__ ptr, const uint32_t *__restrict__ idx,
                                                                const VT *__restrict__ V, uint64_t nrec, uint64_t rows_out,
                                                                double *__restrict__ out, const double *__restrict__ init,
                                                                const double *__restrict__ colw)
{
   constexpr int G = 64 / B;
   const int lane = threadIdx.x & 63, c = lane % B, g = lane / B;
   for (uint64_t r0 = ((uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * G; r0 < rows_out; r0 += (uint64_t)gridDim.x * 4 * G) {
      const uint64_t r = r0 + g;
      double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
      uint32_t p0 = 0, p1 = 0;
      if (r < nrec) {
         p0 = ptr[r];
         p1 = ptr[r + 1];
      }
      // the group's index list in batches of B (one coalesced read, an entry per lane, handed round by shuffles): the row reads of
      // a batch do not wait for any further index read.  (Groups of a wave may run a different number of batches: the shuffles
      // are executed by all lanes, the reads are predicated.)
      uint32_t longest = p1 - p0;
#pragma unroll
      for (int o = 32; o >= B; o >>= 1) longest = max(longest, (uint32_t)__shfl_xor((int)longest, o));
      for (uint32_t base = 0; base < longest; base += B) {
         const uint32_t t = p0 + base + c;
         const int cnt = (int)min((uint32_t)B, p1 - p0 > base ? p1 - p0 - base : 0u);
         const uint32_t mine = t < p1 ? idx[t] : 0u;
#pragma unroll
         for (int e = 0; e < B; e += 4) {
            const uint32_t s0 = (uint32_t)__shfl((int)mine, g * B + e), s1 = (uint32_t)__shfl((int)mine, g * B + e + 1),
                           s2 = (uint32_t)__shfl((int)mine, g * B + e + 2), s3 = (uint32_t)__shfl((int)mine, g * B + e + 3);
            if (e < cnt) a0 += (double)V[(uint64_t)s0 * B + c];
            if (e + 1 < cnt) a1 += (double)V[(uint64_t)s1 * B + c];
            if (e + 2 < cnt) a2 += (double)V[(uint64_t)s2 * B + c];
            if (e + 3 < cnt) a3 += (double)V[(uint64_t)s3 * B + c];
         }
      }
      if (r < rows_out) {
         double a = (a0 + a1) + (a2 + a3);
         if (colw) a *= colw[c] * 32.0;
         out[r * B + c] = init ? init[r * B + c] + a : a;
      }
   }
}

// The gather kernel a launch takes: 1 = k_sparse_rows_sum, 2 = k_sparse_rows_sum_batched, 3 = k_sparse_rows_sum_short (which exists for
// 16 and 32 columns and has no per-row factor: a request for it outside that is served by the batched kernel).
int sparse_rows_sum_variant(int b, bool rowscale, bool short_lists, double avg_len)
{
   // measured (scripts/ab_gather.sh, cfg3): the batched kernel takes 0.3 ms off the K3 gather (short lists per sample),
   // nothing off the K2 one and costs it 6-50 us at the small sizes -- so K3 takes the batched kernel, K2 the plain one.
   // Both sit at ~7 TB/s out of the Infinity Cache; with the gathered matrix resident in L2 the same kernel reaches 9.4 TB/s
   // (scripts/gather_l2_probe.py), which is all an L2-blocked gather order could win.
   static const int forced = FPCA_TEST_ENV("FPCA_GATHER") ? atoi(FPCA_TEST_ENV("FPCA_GATHER")) : 0; // 1 / 2 force one kernel (A/B)
   // 3: several rows per wave, for lists of a dozen entries (measured on the 1/8 shard of cfg3, 12.5 entries per sample: see DESIGN 3c)
   const int variant = forced ? forced : (avg_len > 0 && avg_len <= 24.0 && b <= 32 && !rowscale) ? 3 : ((rowscale || short_lists) ? 2 : 1);
   if (variant == 3 && b <= 32 && !rowscale) return 3;
   return variant == 1 ? 1 : 2;
}

unsigned gather_blocks_beside(const CuFootprint &gemm, int gather_vgprs, int ncu)
{
   constexpr int SIMDS = 4, WAVE_SLOTS = 8, VGPRS = 512, LDS = 160 * 1024; // of a CU: SIMDs, waves and registers of a SIMD, bytes of LDS
   const auto alloc = [](int r) { return (std::max(r, 1) + 7) / 8 * 8; };
   const int wps = std::max((gemm.waves + SIMDS - 1) / SIMDS, 1), regs = alloc(gemm.vgprs) * wps; // of one GEMM workgroup per SIMD
   // the GEMM's workgroups that share a CU (the 3.5-tile 8-wave instance: one, by its LDS; the 2-tile 4-wave one: two)
   const int wgs = std::max(std::min({WAVE_SLOTS / wps, VGPRS / regs, gemm.lds_bytes > 0 ? LDS / gemm.lds_bytes : WAVE_SLOTS}), 1);
   const int slots = WAVE_SLOTS - wgs * wps, left = VGPRS - wgs * regs;
   const int per_cu = std::min(slots, left / alloc(gather_vgprs));
   return (unsigned)std::max(per_cu, 1) * (unsigned)std::max(ncu, 1);
}

// The one-wave-per-row kernels walk the rows in a grid-stride loop, a wave a row: a smaller grid changes no sum.
unsigned sparse_rows_sum_grid(uint64_t rows_out, unsigned block_limit)
{
   const unsigned blocks = (unsigned)std::min<uint64_t>(65536, (rows_out + 3) / 4);
   return block_limit ? std::min(blocks, block_limit) : blocks;
}

// the kernel of (variant 1 / 2, b, VT), for its attributes
template <class VT>
static const void *sparse_rows_sum_kernel(int variant, int b)
{
#define FPCA_GATHER_FN(B_) (variant == 1 ? reinterpret_cast<const void *>(&k_sparse_rows_sum<B_, VT>) : reinterpret_cast<const void *>(&k_sparse_rows_sum_batched<B_, VT>))
   return b == 16 ? FPCA_GATHER_FN(16) : b == 32 ? FPCA_GATHER_FN(32) : b == 64 ? FPCA_GATHER_FN(64) : nullptr;
#undef FPCA_GATHER_FN
}

unsigned sparse_rows_sum_blocks_beside(const CuFootprint &gemm, int b, bool f32, bool rowscale, bool short_lists, double avg_len)
{
   const int variant = sparse_rows_sum_variant(b, rowscale, short_lists, avg_len);
   if (variant == 3) return 0;
   const void *fn = f32 ? sparse_rows_sum_kernel<float>(variant, b) : sparse_rows_sum_kernel<double>(variant, b);
   if (!fn) throw Error(-1, "sparse_rows_sum: block width must be 16, 32 or 64");
   // asked once per kernel (this runs in every apply); the devices of one process are alike
   static std::mutex mtx;
   static std::map<const void *, int> regs_of;
   static int ncu = 0;
   std::lock_guard<std::mutex> lock(mtx);
   auto it = regs_of.find(fn);
   if (it == regs_of.end()) {
      hipFuncAttributes attr;
      if (hipFuncGetAttributes(&attr, fn) != hipSuccess || attr.numRegs <= 0) throw Error(-3, "sparse_rows_sum: the gather kernel's registers could not be read");
      it = regs_of.emplace(fn, attr.numRegs).first;
   }
   if (!ncu) {
      int dev = 0;
      if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || ncu <= 0) {
         ncu = 0;
         throw Error(-3, "sparse_rows_sum: the device's CU count could not be read");
      }
   }
   return gather_blocks_beside(gemm, it->second, ncu);
}

template <class VT>
static void sparse_rows_sum_t(const uint32_t *ptr, const uint32_t *idx, const VT *V, const double *rowscale, int b, uint64_t nrec,
                              uint64_t rows_out, double *out, hipStream_t stream, const double *init, bool short_lists, const double *colw, double avg_len,
                              unsigned block_limit)
{
   if (!rows_out) return;
   // FPCA_GATHER_BLOCKS (test builds, read on every call) replaces the limit on every launch, inline ones too, for the tests and for
   // A/B runs: a number of blocks, 0 for no limit
   if (const char *env_b = FPCA_TEST_ENV("FPCA_GATHER_BLOCKS")) {
      if (atoi(env_b) < 0) throw Error(-1, "FPCA_GATHER_BLOCKS is a number of blocks (0: no limit)");
      block_limit = (unsigned)atoi(env_b);
   }
   const unsigned blocks = sparse_rows_sum_grid(rows_out, block_limit);
   const int variant = sparse_rows_sum_variant(b, rowscale != nullptr, short_lists, avg_len);
   if (FPCA_TEST_ENV("FPCA_GATHER_VERBOSE")) // (test builds: what the tests hold the grid to; the several-rows-per-wave kernel has its own grid)
      std::fprintf(stderr, "[fpca] gather launch: kernel %d, %llu rows, %u blocks, limit %u\n", variant, (unsigned long long)rows_out, blocks, block_limit);
#define FPCA_GATHER_CASE(B_)                                                                                                    \
   case B_:                                                                                                                     \
      if (variant == 3 && B_ <= 32) {                                                                                           \
         const unsigned blocks3 = (unsigned)std::min<uint64_t>(65536, (rows_out + 4 * (64 / B_) - 1) / (4 * (64 / B_)));        \
         hipLaunchKernelGGL((k_sparse_rows_sum_short<(B_ <= 32 ? B_ : 32), VT>), dim3(blocks3), dim3(256), 0, stream, ptr, idx, V, nrec, rows_out, out, init, colw); \
      } else if (variant == 1)                                                                                                  \
         hipLaunchKernelGGL((k_sparse_rows_sum<B_, VT>), dim3(blocks), dim3(256), 0, stream, ptr, idx, V, rowscale, nrec, rows_out, out, init, colw); \
      else                                                                                                                      \
         hipLaunchKernelGGL((k_sparse_rows_sum_batched<B_, VT>), dim3(blocks), dim3(256), 0, stream, ptr, idx, V, rowscale, nrec, rows_out, out, init, colw); \
      break;
   switch (b) {
      FPCA_GATHER_CASE(16)
      FPCA_GATHER_CASE(32)
      FPCA_GATHER_CASE(64)
   default: throw Error(-1, "sparse_rows_sum: block width must be 16, 32 or 64");
   }
#undef FPCA_GATHER_CASE
   launch_check();
}
void sparse_rows_sum(const uint32_t *ptr, const uint32_t *idx, const double *V, const double *rowscale, int b, uint64_t nrec,
                     uint64_t rows_out, double *out, hipStream_t stream, const double *init, bool short_lists, double avg_len, unsigned block_limit)
{
   sparse_rows_sum_t<double>(ptr, idx, V, rowscale, b, nrec, rows_out, out, stream, init, short_lists, nullptr, avg_len, block_limit);
}
void sparse_rows_sum_f32(const uint32_t *ptr, const uint32_t *idx, const float *V, const double *colw, int b, uint64_t nrec, uint64_t rows_out,
                         double *out, hipStream_t stream, const double *init, bool short_lists, double avg_len, unsigned block_limit)
{
   sparse_rows_sum_t<float>(ptr, idx, V, nullptr, b, nrec, rows_out, out, stream, init, short_lists, colw, avg_len, block_limit);
}

// ------------------------------------------------------------------------------------------------
// Helpers of the hybrid missing-indicator route (missing_routes.hip ensure_hybrid): the few SNPs whose missing calls are too many
// for the sparse gathers get their indicator matrix E on the matrix cores, as a compacted sub-matrix.
//   gather_packed_rows  dst[r] = src[idx[r]] (records of `pitch` bytes), rows r >= nidx filled with 0xff = "dosage 0, not missing"
//   patch_missing_rows  in the records idx[r] of `packed`: code 01 (missing) -> 11 (dosage 0): G.M is unchanged, E becomes 0 --
//                       the view of the matrix whose remaining missing calls the sparse lists hold
//   scatter_packed_rows packed[idx[r]] = src[r]  (puts the original records back)
//   gather_scaled_rows  dst[r][c] = V[idx[r]][c] * scale[idx[r]], rows >= nidx zero        (fp64, [.][b])
//   scatter_rows        dst[idx[r]][c] = src[r][c]
__global__ __launch_bounds__(256) void k_gather_packed_rows(const uint8_t *__restrict__ src, size_t pitch, const uint32_t *__restrict__ idx,
                                                             uint32_t nidx, uint8_t *__restrict__ dst)
{
   const u4 *s = blockIdx.x < nidx ? reinterpret_cast<const u4 *>(src + (size_t)idx[blockIdx.x] * pitch) : nullptr;
   u4 *d = reinterpret_cast<u4 *>(dst + (size_t)blockIdx.x * pitch);
   const u4 fill = {0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu};
   for (size_t i = threadIdx.x; i < pitch / 16; i += 256) d[i] = s ? s[i] : fill;
}
__global__ __launch_bounds__(256) void k_patch_missing_rows(uint8_t *__restrict__ packed, size_t pitch, const uint32_t *__restrict__ idx)
{
   u4 *row = reinterpret_cast<u4 *>(packed + (size_t)idx[blockIdx.x] * pitch);
   for (size_t i = threadIdx.x; i < pitch / 16; i += 256) {
      u4 x = row[i];
#pragma unroll
      for (int k = 0; k < 4; k++) x[k] |= (x[k] & ~(x[k] >> 1) & 0x55555555u) << 1;
      row[i] = x;
   }
}
__global__ __launch_bounds__(256) void k_scatter_packed_rows(const uint8_t *__restrict__ src, size_t pitch, const uint32_t *__restrict__ idx,
                                                              uint8_t *__restrict__ packed)
{
   const u4 *s = reinterpret_cast<const u4 *>(src + (size_t)blockIdx.x * pitch);
   u4 *d = reinterpret_cast<u4 *>(packed + (size_t)idx[blockIdx.x] * pitch);
   for (size_t i = threadIdx.x; i < pitch / 16; i += 256) d[i] = s[i];
}
__global__ __launch_bounds__(256) void k_gather_scaled_rows(const double *__restrict__ V, const double *__restrict__ scale,
                                                             const uint32_t *__restrict__ idx, uint32_t nidx, uint64_t rows_out, int b,
                                                             double *__restrict__ dst)
{
   for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < rows_out * b; i += (uint64_t)gridDim.x * 256) {
      const uint64_t r = i / b;
      const int c = (int)(i % b);
      double v = 0.0;
      if (r < nidx) {
         const uint32_t j = idx[r];
         v = V[(uint64_t)j * b + c] * (scale ? scale[j] : 1.0);
      }
      dst[i] = v;
   }
}
__global__ __launch_bounds__(256) void k_scatter_rows(const double *__restrict__ src, const uint32_t *__restrict__ idx, uint32_t nidx, int b,
                                                       double *__restrict__ dst)
{
   for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < (uint64_t)nidx * b; i += (uint64_t)gridDim.x * 256) {
      const uint64_t r = i / b;
      dst[(uint64_t)idx[r] * b + (i % b)] = src[i];
   }
}
void gather_packed_rows(const uint8_t *src, size_t pitch, const uint32_t *idx, uint32_t nidx, uint32_t rows_out, uint8_t *dst, hipStream_t stream)
{
   if (!rows_out) return;
   hipLaunchKernelGGL(k_gather_packed_rows, dim3(rows_out), dim3(256), 0, stream, src, pitch, idx, nidx, dst);
   launch_check();
}
void patch_missing_rows(uint8_t *packed, size_t pitch, const uint32_t *idx, uint32_t nidx, hipStream_t stream)
{
   if (!nidx) return;
   hipLaunchKernelGGL(k_patch_missing_rows, dim3(nidx), dim3(256), 0, stream, packed, pitch, idx);
   launch_check();
}
void scatter_packed_rows(const uint8_t *src, size_t pitch, const uint32_t *idx, uint32_t nidx, uint8_t *packed, hipStream_t stream)
{
   if (!nidx) return;
   hipLaunchKernelGGL(k_scatter_packed_rows, dim3(nidx), dim3(256), 0, stream, src, pitch, idx, packed);
   launch_check();
}
void gather_scaled_rows(const double *V, const double *scale, const uint32_t *idx, uint32_t nidx, uint64_t rows_out, int b, double *dst,
                        hipStream_t stream)
{
   if (!rows_out) return;
   const unsigned blocks = (unsigned)std::min<uint64_t>(4096, (rows_out * b + 255) / 256);
   hipLaunchKernelGGL(k_gather_scaled_rows, dim3(blocks), dim3(256), 0, stream, V, scale, idx, nidx, rows_out, b, dst);
   launch_check();
}
void scatter_rows(const double *src, const uint32_t *idx, uint32_t nidx, int b, double *dst, hipStream_t stream)
{
   if (!nidx) return;
   const unsigned blocks = (unsigned)std::min<uint64_t>(4096, ((uint64_t)nidx * b + 255) / 256);
   hipLaunchKernelGGL(k_scatter_rows, dim3(blocks), dim3(256), 0, stream, src, idx, nidx, b, dst);
   launch_check();
}

} // namespace kern
} // namespace fpca
