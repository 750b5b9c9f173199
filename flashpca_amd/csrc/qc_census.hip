// qc_census.hip -- genotype counts over chosen samples / chosen SNPs, the HWE exact test and the two QC rules on top of them:
// fpca_snp_counts / fpca_sample_counts / fpca_hwe_exact / fpca_sample_qc / fpca_snp_qc_samples (include/fpca.h "Genotype census"),
// fpca_debug_sample_qc_rule / fpca_debug_snp_qc_counts_rule / fpca_bench_qc.
//
// All counts are indexed by the RAW .bed code (0 hom A1, 1 missing, 2 het, 3 hom A2); pad cells are never counted.
//   k_snp_counts     one workgroup per SNP, K1's 16-byte loads and bit-plane popcounts under the keep-bits row of sample_mask.hip (bit 2 s
//                    set for kept sample s; for "all samples" the row has the bits of the N real samples, so the pad cells drop out here
//                    too).  Four uint32 per SNP, one 16-byte store.  HBM-bound like K1: pitch bytes per SNP, the mask row out of L2.
//   k_sample_counts  the column census of the SNP-major matrix.  A workgroup owns a strip of 256 32-bit words of the record (4,096
//                    samples) and a slab of consecutive SNPs; a lane owns ONE word (16 samples) and walks down the slab in groups of 15
//                    records whose loads are all issued before the first is used (a wave instruction reads 256 contiguous bytes of one
//                    record).  A record that the SNP mask leaves out is skipped by a wave-uniform branch on a scalar bit word and counts as
//                    an all-zero word, which has no bit in any of the three planes  lo & ~hi (missing), hi & ~lo (het), lo & hi (hom A2).
//                    The planes are summed in VERTICAL counters -- 16 fields of 2 bits per register take 3 records, 8 fields of 4 bits 15,
//                    4 fields of 8 bits 255, then 32 bits: 3 x (1 + 2 + 4 + 16) = 69 registers, and per sample and SNP a fraction of one
//                    add instead of three.  Code 0 is the number of records counted minus the other three (host).  Slabs are combined with
//                    uint32 atomicAdd (a vector-memory atomic) into a plane-major scratch acc[plane][sample-in-word][word]: for a fixed
//                    plane and sample-in-word the 64 lanes of a wave add to 64 consecutive words, 256 contiguous bytes per instruction.
//                    Integer sums do not depend on the order of arrival: a repeat call is bit-identical.  No LDS, no barrier.
//   k_hwe_exact      one SNP per lane, counts[P][4] -> p[P] in fp64 (Wigginton, Cutler & Abecasis 2005 as restated in include/fpca.h):
//                    first the walk from the mode to the observed heterozygote count, which gives w(a); then the downward and the upward
//                    walk in ONE loop, two independent multiply-divide chains per lane that overlap.  The first walk is short wherever a
//                    SNP is near equilibrium (a is near the mode) and can only be as long as the longer of the other two.  Loop lengths
//                    differ per lane.  No atomics, no LDS; FMA contraction is off in the recurrence.
// No kernel reads a cell outside [0, P_pad) x pitch: records j < P_g only, bytes below pitch only.
// The rules run on the host: a scan over N or P_g entries is not a hot path, and the host's IEEE divide makes the maf decision agree bit for
// bit with snp_qc_rule on K1's mean.
#include <algorithm>
#include <cmath>

#include "ctx.hpp"
#include "launch_check.hpp"

using namespace fpca;

namespace {

constexpr int QC_GROUP = 15;                  // records per load group = what a 4-bit field takes (5 x 3)
constexpr int QC_GROUPS8 = 17;                // groups an 8-bit field takes (17 x 15 = 255)
constexpr uint64_t QC_SLAB_MAX = 16 * QC_GROUP * QC_GROUPS8; // 4,080 records per slab: 48 atomics per lane against 4,080 loads
constexpr uint64_t QC_WANT_WGS = 2048;        // workgroups that fill the device (256 CUs x 8)
constexpr int QC_STRIP = 256;                 // words of the record per workgroup

// the kept samples' counts of one 32-bit word (16 samples) by raw code; m has bit 2 s set for kept sample s
__device__ __forceinline__ void census_word(uint32_t w, uint32_t m, uint32_t &c0, uint32_t &c1, uint32_t &c2, uint32_t &c3)
{
   const uint32_t lo = w & 0x55555555u, hi = (w >> 1) & 0x55555555u;
   c3 += __popc(lo & hi & m);
   c2 += __popc(hi & ~lo & m);
   c1 += __popc(lo & ~hi & m);
   c0 += __popc(~(lo | hi) & m);
}

__global__ __launch_bounds__(256) void k_snp_counts(const uint8_t *__restrict__ packed, size_t pitch, const uint8_t *__restrict__ keep_bits,
                                                     uint4 *__restrict__ counts)
{
   const uint64_t snp = blockIdx.x;
   const uint4 *row = reinterpret_cast<const uint4 *>(packed + snp * pitch);
   const uint4 *mrow = reinterpret_cast<const uint4 *>(keep_bits);
   const uint32_t nvec = (uint32_t)(pitch / 16);
   uint32_t c0 = 0, c1 = 0, c2 = 0, c3 = 0;
   for (uint32_t v = threadIdx.x; v < nvec; v += 256) {
      const uint4 q = row[v], m = mrow[v];
      census_word(q.x, m.x, c0, c1, c2, c3);
      census_word(q.y, m.y, c0, c1, c2, c3);
      census_word(q.z, m.z, c0, c1, c2, c3);
      census_word(q.w, m.w, c0, c1, c2, c3);
   }
   for (int off = 32; off > 0; off >>= 1) {
      c0 += __shfl_down(c0, off);
      c1 += __shfl_down(c1, off);
      c2 += __shfl_down(c2, off);
      c3 += __shfl_down(c3, off);
   }
   __shared__ uint32_t red[4][4];
   const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
   if (lane == 0) {
      red[wave][0] = c0;
      red[wave][1] = c1;
      red[wave][2] = c2;
      red[wave][3] = c3;
   }
   __syncthreads();
   if (threadIdx.x == 0)
      counts[snp] = make_uint4(red[0][0] + red[1][0] + red[2][0] + red[3][0], red[0][1] + red[1][1] + red[2][1] + red[3][1],
                               red[0][2] + red[1][2] + red[2][2] + red[3][2], red[0][3] + red[1][3] + red[2][3] + red[3][3]);
}

// snp_bits (MASKED): bit j % 32 of word j / 32 set for a counted record j, one spare word behind the last; acc: [3][16][nwords]
template <bool MASKED>
__global__ __launch_bounds__(256) void k_sample_counts(const uint32_t *__restrict__ packed, uint32_t nwords, uint32_t nstrips,
                                                        const uint32_t *__restrict__ snp_bits, uint64_t P, uint64_t slab, uint32_t *__restrict__ acc)
{
   const uint32_t strip = blockIdx.x % nstrips;
   const uint64_t sl = blockIdx.x / nstrips;
   const uint32_t word = strip * QC_STRIP + threadIdx.x;
   if (word >= nwords) return; // (the kernel has no barrier)
   const uint64_t j0 = sl * slab, j1 = j0 + slab < P ? j0 + slab : P;
   const uint32_t *col = packed + word; // record j of this lane's word: col[j * nwords]
   uint32_t c32[3][16];
#pragma unroll
   for (int p = 0; p < 3; p++)
#pragma unroll
      for (int s = 0; s < 16; s++) c32[p][s] = 0;
   for (uint64_t j = j0; j < j1;) {
      uint32_t c8[3][4];
#pragma unroll
      for (int p = 0; p < 3; p++)
#pragma unroll
         for (int q = 0; q < 4; q++) c8[p][q] = 0;
      for (int g = 0; g < QC_GROUPS8 && j < j1; g++, j += QC_GROUP) {
         const uint32_t cnt = j1 - j < QC_GROUP ? (uint32_t)(j1 - j) : (uint32_t)QC_GROUP;
         // which of the group's records count (wave-uniform: j depends on the workgroup and the trip count only)
         uint32_t take = cnt == QC_GROUP ? 0x7FFFu : (1u << cnt) - 1u;
         if (MASKED) {
            const uint64_t two = (uint64_t)snp_bits[j >> 5] | ((uint64_t)snp_bits[(j >> 5) + 1] << 32);
            take &= (uint32_t)(two >> (j & 31));
         }
         uint32_t w[QC_GROUP];
#pragma unroll
         for (int t = 0; t < QC_GROUP; t++) {
            w[t] = 0; // a record left out reads as sixteen times code 0: no bit in any plane
            if ((take >> t) & 1u) w[t] = col[(size_t)(j + t) * nwords];
         }
         uint32_t c4[3][2];
#pragma unroll
         for (int p = 0; p < 3; p++) c4[p][0] = c4[p][1] = 0;
#pragma unroll
         for (int t3 = 0; t3 < QC_GROUP; t3 += 3) {
            uint32_t c2[3] = {0, 0, 0};
#pragma unroll
            for (int u = 0; u < 3; u++) {
               const uint32_t lo = w[t3 + u] & 0x55555555u, hi = (w[t3 + u] >> 1) & 0x55555555u;
               c2[0] += lo & ~hi;
               c2[1] += hi & ~lo;
               c2[2] += lo & hi;
            }
#pragma unroll
            for (int p = 0; p < 3; p++) { // field t of c4[p][e] is sample 2 t + e
               c4[p][0] += c2[p] & 0x33333333u;
               c4[p][1] += (c2[p] >> 2) & 0x33333333u;
            }
         }
#pragma unroll
         for (int p = 0; p < 3; p++) { // byte u of c8[p][q] is sample 4 u + {0, 2, 1, 3}[q]
            c8[p][0] += c4[p][0] & 0x0F0F0F0Fu;
            c8[p][1] += (c4[p][0] >> 4) & 0x0F0F0F0Fu;
            c8[p][2] += c4[p][1] & 0x0F0F0F0Fu;
            c8[p][3] += (c4[p][1] >> 4) & 0x0F0F0F0Fu;
         }
      }
#pragma unroll
      for (int p = 0; p < 3; p++)
#pragma unroll
         for (int u = 0; u < 4; u++) {
            c32[p][4 * u + 0] += (c8[p][0] >> (8 * u)) & 0xFFu;
            c32[p][4 * u + 2] += (c8[p][1] >> (8 * u)) & 0xFFu;
            c32[p][4 * u + 1] += (c8[p][2] >> (8 * u)) & 0xFFu;
            c32[p][4 * u + 3] += (c8[p][3] >> (8 * u)) & 0xFFu;
         }
   }
#pragma unroll
   for (int p = 0; p < 3; p++)
#pragma unroll
      for (int s = 0; s < 16; s++) atomicAdd(acc + (size_t)(p * 16 + s) * nwords + word, c32[p][s]);
}

// one step of the recurrence from heterozygote count h (include/fpca.h, steps 5 - 7); r, n, h are integers held in fp64
__device__ __forceinline__ double hwe_down(double w, double h, double r, double n)
{
#pragma clang fp contract(off)
   const double hr = (r - h) * 0.5, hc = n - h - hr;
   const double num = h * (h - 1.0), den = 4.0 * (hr + 1.0) * (hc + 1.0);
   const double t = w * num;
   return t / den;
}

__device__ __forceinline__ double hwe_up(double w, double h, double r, double n)
{
#pragma clang fp contract(off)
   const double hr = (r - h) * 0.5, hc = n - h - hr;
   const double num = 4.0 * hr * hc, den = (h + 2.0) * (h + 1.0);
   const double t = w * num;
   return t / den;
}

__global__ __launch_bounds__(256) void k_hwe_exact(const uint4 *__restrict__ counts, uint64_t P, double *__restrict__ pval)
{
#pragma clang fp contract(off)
   const uint64_t snp = (uint64_t)blockIdx.x * 256 + threadIdx.x;
   if (snp >= P) return;
   const uint4 q = counts[snp];
   const uint64_t a = q.z, b = q.x < q.w ? q.x : q.w, c = q.x < q.w ? q.w : q.x, n = a + b + c, r = 2 * b + a;
   if (n == 0) {
      pval[snp] = 1.0;
      return;
   }
   uint64_t mid = r * (2 * n - r) / (2 * n); // (r <= n < 2^32: the product stays below 2^64)
   if ((mid ^ r) & 1) mid++;
   const double rd = (double)r, nd = (double)n, ad = (double)a, md = (double)mid;
   // the term of the observed count
   double wa = 1.0;
   if (ad < md)
      for (double h = md; h > ad && wa > 0.0; h -= 2.0) wa = hwe_down(wa, h, rd, nd);
   else
      for (double h = md; h < ad && wa > 0.0; h += 2.0) wa = hwe_up(wa, h, rd, nd);
   const double thr = wa * (1.0 + 0x1p-20);
   // both walks away from the mode at once; a walk ends at its last count or at a term that is exactly 0
   double tot = 1.0, tail = 1.0 <= thr ? 1.0 : 0.0;
   double wd = 1.0, hd = md, wu = 1.0, hu = md;
   bool down = hd >= 2.0, up = hu <= rd - 2.0;
   while (down || up) {
      if (down) {
         wd = hwe_down(wd, hd, rd, nd);
         hd -= 2.0;
         tot += wd;
         tail += wd <= thr ? wd : 0.0;
         down = hd >= 2.0 && wd > 0.0;
      }
      if (up) {
         wu = hwe_up(wu, hu, rd, nd);
         hu += 2.0;
         tot += wu;
         tail += wu <= thr ? wu : 0.0;
         up = hu <= rd - 2.0 && wu > 0.0;
      }
   }
   const double p = tail / tot;
   pval[snp] = p < 1.0 ? p : 1.0;
}

// what every entry point refuses (before any device work)
void qc_refuse(const fpca_ctx *c, const char *fn)
{
   if (!c) throw Error(FPCA_EINVAL, std::string("bad argument to ") + fn + " (NULL context)");
   if (c->dense)
      throw Error(FPCA_EINVAL, std::string(fn) + ": this context holds a dense matrix; genotype counts exist for packed genotypes only (fpca_create, "
                                                 "fpca_create_from_bed, synthetic)");
   if (c->multi() || (c->rank_known && c->nranks > 1))
      throw Error(FPCA_EINVAL, std::string(fn) + ": this context is one shard of several (a communicator, an all-reduce hook or fpca_set_rank with "
                                                 "more than one rank); the counts are over all SNPs -- take them on a single context");
   if (c->masked())
      throw Error(FPCA_EINVAL, std::string(fn) + ": a sample mask is set (fpca_set_sample_mask); clear it and pass the mask as the `samples` argument "
                                                 "instead");
   if (c->N > 0xFFFFFFFFull || c->P_g > 0xFFFFFFFFull)
      throw Error(FPCA_EINVAL, std::string(fn) + ": " + std::to_string(c->N) + " samples x " + std::to_string(c->P_g) +
                                  " SNPs; the counts are 32-bit, both must stay below 2^32");
}

void check_mind(const char *fn, double max_missing)
{
   if (std::isnan(max_missing)) throw Error(FPCA_EINVAL, std::string(fn) + ": max_missing is NaN");
   if (max_missing < 0) throw Error(FPCA_EINVAL, std::string(fn) + ": max_missing = " + std::to_string(max_missing) + " is negative");
}

void check_hwe(const char *fn, double min_hwe_p)
{
   if (std::isnan(min_hwe_p)) throw Error(FPCA_EINVAL, std::string(fn) + ": min_hwe_p is NaN");
   if (min_hwe_p > 1) throw Error(FPCA_EINVAL, std::string(fn) + ": min_hwe_p = " + std::to_string(min_hwe_p) + " is above 1, the largest p-value there is");
}

uint64_t count_nonzero(const uint8_t *m, uint64_t n, uint64_t all)
{
   if (!m) return all;
   uint64_t k = 0;
   for (uint64_t i = 0; i < n; i++) k += m[i] != 0;
   return k;
}

// the keep-bits row of the per-SNP pass on the device: `samples` (NULL: all N), nothing at or after sample N
DevMem<uint8_t> upload_keep_bits(fpca_ctx *c, const uint8_t *samples, const char *fn)
{
   std::vector<uint8_t> bits(c->pitch, 0);
   for (uint64_t i = 0; i < c->N; i++)
      if (!samples || samples[i]) bits[i / 4] |= (uint8_t)(1u << (2 * (i % 4)));
   DevMem<uint8_t> d(bits.size(), fn, "the mask row of the count pass");
   HIP_CHECK(hipMemcpyAsync(d.p, bits.data(), bits.size(), hipMemcpyHostToDevice, c->stream));
   HIP_CHECK(hipStreamSynchronize(c->stream)); // (the host vector goes out of scope)
   return d;
}

void launch_snp_counts(const fpca_ctx *c, const uint8_t *d_bits, uint32_t *d_counts)
{
   if (!c->P_g) return;
   hipLaunchKernelGGL(k_snp_counts, dim3((unsigned)c->P_g), dim3(256), 0, c->stream, c->d_packed, c->pitch, d_bits, reinterpret_cast<uint4 *>(d_counts));
   launch_check();
}

void launch_hwe(const fpca_ctx *c, const uint32_t *d_counts, uint64_t n, double *d_p)
{
   if (!n) return;
   hipLaunchKernelGGL(k_hwe_exact, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, reinterpret_cast<const uint4 *>(d_counts), n, d_p);
   launch_check();
}

// the plan and the scratch of the per-sample pass
struct SampleCensus {
   uint32_t nwords = 0, nstrips = 0;
   uint64_t slab = 0, nslabs = 0;
   DevMem<uint32_t> d_bits, d_acc;
   bool masked = false;
   size_t acc_words() const { return (size_t)48 * nwords; }
};

void sample_census_plan(const fpca_ctx *c, SampleCensus &s)
{
   s.nwords = (uint32_t)(c->pitch / 4);
   s.nstrips = (s.nwords + QC_STRIP - 1) / QC_STRIP;
   const uint64_t P = c->P_g, want = (QC_WANT_WGS + s.nstrips - 1) / s.nstrips, period = (uint64_t)QC_GROUP * QC_GROUPS8;
   s.slab = std::min<uint64_t>(QC_SLAB_MAX, std::max<uint64_t>(period, round_up((P + want - 1) / want, period)));
   if (const char *v = FPCA_TEST_ENV("FPCA_QC_SLAB_SNPS"))
      if (std::atoll(v) > 0) s.slab = (uint64_t)std::atoll(v);
   while ((P + s.slab - 1) / s.slab * s.nstrips > (1ull << 30)) s.slab *= 2; // one launch
   s.nslabs = (P + s.slab - 1) / s.slab;
}

void sample_census_alloc(fpca_ctx *c, SampleCensus &s, const uint8_t *snps, const char *fn)
{
   sample_census_plan(c, s);
   s.d_acc = DevMem<uint32_t>(s.acc_words(), fn, "the per-sample count planes");
   s.masked = snps != nullptr;
   if (snps) {
      std::vector<uint32_t> bits(c->P_g / 32 + 2, 0);
      for (uint64_t j = 0; j < c->P_g; j++)
         if (snps[j]) bits[j >> 5] |= 1u << (j & 31);
      s.d_bits = DevMem<uint32_t>(bits.size(), fn, "the SNP mask of the count pass");
      HIP_CHECK(hipMemcpyAsync(s.d_bits.p, bits.data(), bits.size() * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
      HIP_CHECK(hipStreamSynchronize(c->stream));
   }
}

void launch_sample_counts(const fpca_ctx *c, const SampleCensus &s)
{
   HIP_CHECK(hipMemsetAsync(s.d_acc.p, 0, s.acc_words() * sizeof(uint32_t), c->stream));
   if (!s.nslabs) return;
   const dim3 grid((unsigned)(s.nslabs * s.nstrips));
   const uint32_t *packed = reinterpret_cast<const uint32_t *>(c->d_packed);
   if (s.masked)
      hipLaunchKernelGGL(k_sample_counts<true>, grid, dim3(QC_STRIP), 0, c->stream, packed, s.nwords, s.nstrips, s.d_bits.p, c->P_g, s.slab, s.d_acc.p);
   else
      hipLaunchKernelGGL(k_sample_counts<false>, grid, dim3(QC_STRIP), 0, c->stream, packed, s.nwords, s.nstrips, s.d_bits.p, c->P_g, s.slab, s.d_acc.p);
   launch_check();
}

// counts[N][4] by raw code over the SNPs of `snps` (NULL: all); returns the number of SNPs counted
uint64_t sample_counts(fpca_ctx *c, const uint8_t *snps, uint32_t *counts, const char *fn)
{
   const uint64_t n_snps = count_nonzero(snps, c->P_g, c->P_g);
   HIP_CHECK(hipSetDevice(c->device));
   SampleCensus s;
   sample_census_alloc(c, s, snps, fn);
   launch_sample_counts(c, s);
   std::vector<uint32_t> acc(s.acc_words());
   HIP_CHECK(hipMemcpyAsync(acc.data(), s.d_acc.p, acc.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
   HIP_CHECK(hipStreamSynchronize(c->stream));
   for (uint64_t i = 0; i < c->N; i++) {
      const size_t at = (size_t)(i % 16) * s.nwords + i / 16, plane = (size_t)16 * s.nwords;
      const uint32_t c1 = acc[at], c2 = acc[plane + at], c3 = acc[2 * plane + at];
      counts[4 * i + 0] = (uint32_t)(n_snps - c1 - c2 - c3);
      counts[4 * i + 1] = c1;
      counts[4 * i + 2] = c2;
      counts[4 * i + 3] = c3;
   }
   return n_snps;
}

} // namespace

namespace fpca {

uint64_t sample_qc_rule(const uint32_t *counts, uint64_t n_snps, uint64_t N, double max_missing, uint8_t *samples)
{
   const bool by_miss = max_missing < 1;
   uint64_t kept = 0;
   for (uint64_t i = 0; i < N; i++) {
      if (!samples[i]) continue;
      const bool ok = !(by_miss && (double)counts[4 * i + 1] / (double)n_snps > max_missing);
      samples[i] = ok ? 1 : 0;
      kept += ok;
   }
   return kept;
}

uint64_t snp_qc_counts_rule(const uint32_t *counts, const double *p_hwe, uint64_t n, uint64_t P, double min_maf, double max_missing, double min_hwe_p,
                            uint8_t *keep)
{
   const bool by_maf = min_maf > 0, by_miss = max_missing < 1, by_hwe = min_hwe_p > 0;
   uint64_t kept = 0;
   for (uint64_t j = 0; j < P; j++) {
      if (!keep[j]) continue;
      const uint32_t *q = counts + 4 * j;
      bool ok = true;
      if (by_maf) { // K1's arithmetic (k_bed_stats), then snp_qc_rule's
         const uint64_t ngood = (uint64_t)q[0] + q[2] + q[3];
         const double mean = (double)(2 * (uint64_t)q[0] + q[2]) / (double)ngood;
         const double p = mean / 2.0;
         const double maf = ngood == 0 ? 0.0 : std::min(p, 1.0 - p);
         if (maf < min_maf) ok = false;
      }
      if (by_miss && (double)q[1] / (double)n > max_missing) ok = false;
      if (by_hwe && p_hwe[j] < min_hwe_p) ok = false;
      keep[j] = ok ? 1 : 0;
      kept += ok;
   }
   return kept;
}

} // namespace fpca

extern "C" int fpca_snp_counts(fpca_ctx *ctx, const uint8_t *samples, uint32_t *counts)
{
   return guarded([&] {
      static const char *FN = "fpca_snp_counts";
      qc_refuse(ctx, FN);
      if (!counts) throw Error(FPCA_EINVAL, "bad argument to fpca_snp_counts (counts is NULL)");
      if (!ctx->P_g) return;
      HIP_CHECK(hipSetDevice(ctx->device));
      DevMem<uint8_t> d_bits = upload_keep_bits(ctx, samples, FN);
      DevMem<uint32_t> d_counts(ctx->P_g * 4, FN, "the per-SNP counts");
      launch_snp_counts(ctx, d_bits.p, d_counts.p);
      HIP_CHECK(hipMemcpyAsync(counts, d_counts.p, ctx->P_g * 4 * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
      HIP_CHECK(hipStreamSynchronize(ctx->stream));
   });
}

extern "C" int fpca_sample_counts(fpca_ctx *ctx, const uint8_t *snps, uint32_t *counts)
{
   return guarded([&] {
      qc_refuse(ctx, "fpca_sample_counts");
      if (!counts) throw Error(FPCA_EINVAL, "bad argument to fpca_sample_counts (counts is NULL)");
      sample_counts(ctx, snps, counts, "fpca_sample_counts");
   });
}

extern "C" int fpca_hwe_exact(fpca_ctx *ctx, const uint32_t *counts, uint64_t n, double *p)
{
   return guarded([&] {
      static const char *FN = "fpca_hwe_exact";
      qc_refuse(ctx, FN);
      if (n && (!counts || !p)) throw Error(FPCA_EINVAL, std::string("bad argument to fpca_hwe_exact (") + (!counts ? "counts" : "p") + " is NULL)");
      if (n > 0xFFFFFFFFull) throw Error(FPCA_EINVAL, "fpca_hwe_exact: " + std::to_string(n) + " rows of counts; at most 2^32 - 1 in one call");
      if (!n) return;
      HIP_CHECK(hipSetDevice(ctx->device));
      DevMem<uint32_t> d_counts(n * 4, FN, "the counts");
      DevMem<double> d_p(n, FN, "the p-values");
      HIP_CHECK(hipMemcpyAsync(d_counts.p, counts, n * 4 * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
      launch_hwe(ctx, d_counts.p, n, d_p.p);
      HIP_CHECK(hipMemcpyAsync(p, d_p.p, n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
      HIP_CHECK(hipStreamSynchronize(ctx->stream));
   });
}

extern "C" int fpca_sample_qc(fpca_ctx *ctx, const uint8_t *snps, double max_missing, uint8_t *samples, uint64_t *n_kept)
{
   return guarded([&] {
      static const char *FN = "fpca_sample_qc";
      qc_refuse(ctx, FN);
      if (!samples) throw Error(FPCA_EINVAL, "bad argument to fpca_sample_qc (samples is NULL)");
      check_mind(FN, max_missing);
      if (count_nonzero(snps, ctx->P_g, ctx->P_g) == 0)
         throw Error(FPCA_EINVAL, "fpca_sample_qc: no SNP is counted (the mask keeps 0 of " + std::to_string(ctx->P_g) + "); a missing rate needs at least 1");
      std::vector<uint32_t> counts(ctx->N * 4);
      const uint64_t n_snps = sample_counts(ctx, snps, counts.data(), FN);
      const uint64_t kept = sample_qc_rule(counts.data(), n_snps, ctx->N, max_missing, samples);
      if (n_kept) *n_kept = kept;
   });
}

extern "C" int fpca_snp_qc_samples(fpca_ctx *ctx, const uint8_t *samples, double min_maf, double max_missing, double min_hwe_p, uint8_t *snps,
                                   uint64_t *n_kept)
{
   return guarded([&] {
      static const char *FN = "fpca_snp_qc_samples";
      qc_refuse(ctx, FN);
      if (!snps) throw Error(FPCA_EINVAL, "bad argument to fpca_snp_qc_samples (snps is NULL)");
      snp_qc_check_thresholds(FN, min_maf, max_missing);
      check_hwe(FN, min_hwe_p);
      const uint64_t n = count_nonzero(samples, ctx->N, ctx->N), P = ctx->P_g;
      if (n == 0) throw Error(FPCA_EINVAL, "fpca_snp_qc_samples: the sample mask keeps 0 of " + std::to_string(ctx->N) + " samples; frequencies need at least 1");
      const bool by_hwe = min_hwe_p > 0;
      std::vector<uint32_t> counts(P * 4);
      std::vector<double> pv(by_hwe ? P : 0);
      if (P) {
         HIP_CHECK(hipSetDevice(ctx->device));
         DevMem<uint8_t> d_bits = upload_keep_bits(ctx, samples, FN);
         DevMem<uint32_t> d_counts(P * 4, FN, "the per-SNP counts");
         DevMem<double> d_p(by_hwe ? P : 0, FN, "the p-values");
         launch_snp_counts(ctx, d_bits.p, d_counts.p);
         HIP_CHECK(hipMemcpyAsync(counts.data(), d_counts.p, P * 4 * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
         if (by_hwe) {
            launch_hwe(ctx, d_counts.p, P, d_p.p); // straight from the device's counts
            HIP_CHECK(hipMemcpyAsync(pv.data(), d_p.p, P * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
         }
         HIP_CHECK(hipStreamSynchronize(ctx->stream));
      }
      const uint64_t kept = snp_qc_counts_rule(counts.data(), by_hwe ? pv.data() : nullptr, n, P, min_maf, max_missing, min_hwe_p, snps);
      if (n_kept) *n_kept = kept;
   });
}

extern "C" int fpca_debug_sample_qc_rule(const uint32_t *counts, uint64_t n_snps, uint64_t N, double max_missing, uint8_t *samples, uint64_t *n_kept)
{
   return guarded([&] {
      if (!samples || (N && !counts)) throw Error(FPCA_EINVAL, "bad argument to fpca_debug_sample_qc_rule");
      check_mind("fpca_debug_sample_qc_rule", max_missing);
      if (n_snps == 0) throw Error(FPCA_EINVAL, "fpca_debug_sample_qc_rule: no SNP is counted; a missing rate needs at least 1");
      const uint64_t kept = sample_qc_rule(counts, n_snps, N, max_missing, samples);
      if (n_kept) *n_kept = kept;
   });
}

extern "C" int fpca_debug_snp_qc_counts_rule(const uint32_t *counts, const double *p_hwe, uint64_t n, uint64_t P, double min_maf, double max_missing,
                                             double min_hwe_p, uint8_t *keep, uint64_t *n_kept)
{
   return guarded([&] {
      static const char *FN = "fpca_debug_snp_qc_counts_rule";
      if (!keep || (P && !counts) || n == 0) throw Error(FPCA_EINVAL, "bad argument to fpca_debug_snp_qc_counts_rule");
      snp_qc_check_thresholds(FN, min_maf, max_missing);
      check_hwe(FN, min_hwe_p);
      if (min_hwe_p > 0 && P && !p_hwe) throw Error(FPCA_EINVAL, "fpca_debug_snp_qc_counts_rule: min_hwe_p is set and p_hwe is NULL");
      const uint64_t kept = snp_qc_counts_rule(counts, p_hwe, n, P, min_maf, max_missing, min_hwe_p, keep);
      if (n_kept) *n_kept = kept;
   });
}

extern "C" int fpca_bench_qc(fpca_ctx *ctx, int reps, double *ms, double *hwe_steps)
{
   return guarded([&] {
      static const char *FN = "fpca_bench_qc";
      qc_refuse(ctx, FN);
      if (!ms || reps < 1) throw Error(FPCA_EINVAL, "bad argument to fpca_bench_qc");
      const uint64_t P = ctx->P_g;
      if (!P) throw Error(FPCA_EINVAL, "fpca_bench_qc: the context has no SNP");
      HIP_CHECK(hipSetDevice(ctx->device));
      DevMem<uint8_t> d_bits = upload_keep_bits(ctx, nullptr, FN);
      DevMem<uint32_t> d_counts(P * 4, FN, "the per-SNP counts");
      DevMem<double> d_p(P, FN, "the p-values");
      SampleCensus s;
      sample_census_alloc(ctx, s, nullptr, FN);
      ms[0] = time_launches(ctx->stream, FN, 1, reps, [&] { launch_snp_counts(ctx, d_bits.p, d_counts.p); });
      ms[1] = time_launches(ctx->stream, FN, 1, reps, [&] { launch_sample_counts(ctx, s); });
      ms[2] = time_launches(ctx->stream, FN, 1, reps, [&] { launch_hwe(ctx, d_counts.p, P, d_p.p); });
      if (hwe_steps) { // the recurrence steps one launch makes, replayed from the counts: the walk to a, then both walks to their ends
         std::vector<uint32_t> h(P * 4);
         HIP_CHECK(hipMemcpy(h.data(), d_counts.p, P * 4 * sizeof(uint32_t), hipMemcpyDeviceToHost));
         double steps = 0;
         for (uint64_t j = 0; j < P; j++) {
            const uint64_t a = h[4 * j + 2], b = std::min(h[4 * j], h[4 * j + 3]), c = std::max(h[4 * j], h[4 * j + 3]), n = a + b + c, r = 2 * b + a;
            if (!n) continue;
            uint64_t mid = r * (2 * n - r) / (2 * n);
            if ((mid ^ r) & 1) mid++;
            steps += (double)((a > mid ? a - mid : mid - a) / 2 + r / 2); // (an upper figure: a walk that underflows to 0 ends early)
         }
         *hwe_steps = steps;
      }
   });
}
