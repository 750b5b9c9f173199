// snp_subset.hip -- SNP subsets: fpca_snp_missing / fpca_snp_qc / fpca_create_snp_subset (include/fpca.h "SNP subset").
//
// A subset of the SNPs is a NEW context whose packed matrix holds the kept records of the source, in order, in exactly the layout
// fpca_create builds from the re-packed records (same pitch, records [P_kept, P_pad) 0x55, pad bits of the last byte "01").  Every other
// entry point then runs on it unchanged: no GEMM, no missing-call route and no solver knows that the context was compacted.
//   k_gather_records   dst[j][:] = src[idx[j]][:] over pitch bytes, idx ascending.  The destination records are consecutive and of the
//                      source's pitch, so the destination is ONE contiguous stream of P_kept * pitch / 16 sixteen-byte vectors; the grid
//                      tiles that stream in 16 KiB pieces (1,024 vectors: 256 threads x 4).  A tile is a chunk of one long record or a run
//                      of short ones -- the (record, chunk) space in row-major order -- so a 125 KB record and a 128-byte one fill the
//                      device alike, and there is no tail: pitch is a multiple of 128.  Every thread issues its four 16-byte loads before
//                      its four stores (16 KiB in flight per workgroup, eight waves per SIMD at 26 VGPRs).  HBM-bound: pitch * P_kept
//                      bytes read, as many written; the index is read through L2 (one 4-byte word per 16-byte vector, the same word for
//                      every lane of a long record).  Nothing is written at or after record P_kept: those are ctx_alloc_common's 0x55.
// The QC rule (MAF, call rate) runs on the host from K1's per-SNP mean and missing count (snp_qc_rule): a P-entry scan is not a hot
// path, and the host's IEEE divide makes the decision reproducible bit for bit from the oracle's meansd().
#include <algorithm>
#include <cmath>

#include "ctx.hpp"
#include "launch_check.hpp"

using namespace fpca;

namespace {

constexpr int GATHER_UNROLL = 4;
constexpr uint32_t GATHER_TILE = 256 * GATHER_UNROLL; // 16-byte vectors per workgroup

// vpr: 16-byte vectors per record (pitch / 16); total: P_kept * vpr
__global__ __launch_bounds__(256) void k_gather_records(const uint8_t *__restrict__ src, const uint32_t *__restrict__ idx, uint32_t vpr, uint64_t total,
                                                         uint4 *__restrict__ dst)
{
   const uint64_t s0 = (uint64_t)blockIdx.x * GATHER_TILE;
   const uint64_t rec0 = s0 / vpr; // (the same in every lane: one scalar division per workgroup)
   const uint32_t off0 = (uint32_t)(s0 - rec0 * vpr);
   const size_t pitch = (size_t)vpr * 16;
   // every tile but the last is whole (a uniform branch): four index words, then four 16-byte vectors, in flight before the first store
   if (s0 + GATHER_TILE <= total) {
      uint32_t rec[GATHER_UNROLL], off[GATHER_UNROLL];
#pragma unroll
      for (int u = 0; u < GATHER_UNROLL; u++) {
         const uint32_t o = off0 + (uint32_t)u * 256 + threadIdx.x, r = o / vpr; // (o < 1,024 + vpr: 32-bit)
         rec[u] = idx[rec0 + r];
         off[u] = o - r * vpr;
      }
      uint4 v[GATHER_UNROLL];
#pragma unroll
      for (int u = 0; u < GATHER_UNROLL; u++) v[u] = reinterpret_cast<const uint4 *>(src + (size_t)rec[u] * pitch)[off[u]];
#pragma unroll
      for (int u = 0; u < GATHER_UNROLL; u++) dst[s0 + (uint32_t)u * 256 + threadIdx.x] = v[u];
      return;
   }
   for (uint32_t t = threadIdx.x; s0 + t < total; t += 256) {
      const uint32_t o = off0 + t, r = o / vpr;
      dst[s0 + t] = reinterpret_cast<const uint4 *>(src + (size_t)idx[rec0 + r] * pitch)[o - r * vpr];
   }
}

// the calls that read K1's all-sample counts: what they refuse
void refuse_without_counts(const fpca_ctx *c, const char *fn)
{
   if (!c) throw Error(FPCA_EINVAL, std::string("bad argument to ") + fn + " (NULL context)");
   if (c->dense)
      throw Error(FPCA_EINVAL, std::string(fn) + ": this context holds a dense matrix; per-SNP missing counts exist for packed genotypes only "
                                                 "(fpca_create, fpca_create_from_bed, synthetic)");
   if (c->masked())
      throw Error(FPCA_EINVAL, std::string(fn) + ": a sample mask is set (fpca_set_sample_mask); the per-SNP counts are those of all N samples, the "
                                                 "frequencies would be those of the kept ones -- clear the mask first");
   if (c->meansd_preloaded)
      throw Error(FPCA_EINVAL, std::string(fn) + ": this context carries a preloaded mean/sd (fpca_set_meansd); K1 never counted its missing calls");
}

void check_thresholds(const char *fn, double min_maf, double max_missing)
{
   if (std::isnan(min_maf) || std::isnan(max_missing)) throw Error(FPCA_EINVAL, std::string(fn) + ": a threshold is NaN");
   if (min_maf > 0.5)
      throw Error(FPCA_EINVAL, std::string(fn) + ": min_maf = " + std::to_string(min_maf) + " is above 0.5, the largest minor-allele frequency there is");
   if (max_missing < 0) throw Error(FPCA_EINVAL, std::string(fn) + ": max_missing = " + std::to_string(max_missing) + " is negative");
}

} // namespace

namespace fpca {
// the ascending list of the kept records (32-bit record numbers: the kernel's index words)
std::vector<uint32_t> kept_indices(const uint8_t *keep, uint64_t P)
{
   if (P > 0xFFFFFFFFull) throw Error(FPCA_EINVAL, "SNP subsets index records with 32 bits; this context has " + std::to_string(P) + " SNPs");
   std::vector<uint32_t> idx;
   for (uint64_t j = 0; j < P; j++)
      if (keep[j]) idx.push_back((uint32_t)j);
   return idx;
}

namespace kern {
void gather_records(const uint8_t *src, size_t pitch, const uint32_t *idx, uint64_t nrec, uint8_t *dst, hipStream_t stream)
{
   if (!nrec) return;
   const uint32_t vpr = (uint32_t)(pitch / 16);
   const uint64_t total = nrec * vpr;
   hipLaunchKernelGGL(k_gather_records, dim3((unsigned)((total + GATHER_TILE - 1) / GATHER_TILE)), dim3(256), 0, stream, src, idx, vpr, total,
                      reinterpret_cast<uint4 *>(dst));
   launch_check();
}
} // namespace kern

uint64_t snp_qc_rule(const double *mean, const uint32_t *n_missing, uint64_t N, uint64_t P, double min_maf, double max_missing, uint8_t *keep)
{
   const bool by_maf = min_maf > 0, by_miss = max_missing < 1;
   uint64_t kept = 0;
   for (uint64_t j = 0; j < P; j++) {
      if (!keep[j]) continue;
      bool ok = true;
      if (by_maf) {
         const double p = mean[j] / 2.0;
         // (a SNP without a single call has mean 0 / 0: it counts as maf 0)
         const double maf = (n_missing[j] >= N || std::isnan(p)) ? 0.0 : std::min(p, 1.0 - p);
         if (maf < min_maf) ok = false;
      }
      if (by_miss && (double)n_missing[j] / (double)N > max_missing) ok = false;
      keep[j] = ok ? 1 : 0;
      kept += ok;
   }
   return kept;
}

void snp_qc_check_thresholds(const char *fn, double min_maf, double max_missing) { check_thresholds(fn, min_maf, max_missing); }

} // namespace fpca

extern "C" int fpca_snp_missing(fpca_ctx *ctx, uint32_t *n_missing)
{
   return guarded([&] {
      refuse_without_counts(ctx, "fpca_snp_missing");
      if (!n_missing) throw Error(FPCA_EINVAL, "bad argument to fpca_snp_missing (n_missing is NULL)");
      HIP_CHECK(hipSetDevice(ctx->device));
      ensure_stats(ctx);
      std::copy(ctx->h_nmiss.begin(), ctx->h_nmiss.end(), n_missing);
   });
}

extern "C" int fpca_snp_qc(fpca_ctx *ctx, double min_maf, double max_missing, uint8_t *keep, uint64_t *n_kept)
{
   return guarded([&] {
      refuse_without_counts(ctx, "fpca_snp_qc");
      if (!keep) throw Error(FPCA_EINVAL, "bad argument to fpca_snp_qc (keep is NULL)");
      check_thresholds("fpca_snp_qc", min_maf, max_missing);
      HIP_CHECK(hipSetDevice(ctx->device));
      ensure_stats(ctx);
      std::vector<double> mean(ctx->P_g);
      if (ctx->P_g) HIP_CHECK(hipMemcpy(mean.data(), ctx->d_mean, ctx->P_g * sizeof(double), hipMemcpyDeviceToHost));
      const uint64_t kept = snp_qc_rule(mean.data(), ctx->h_nmiss.data(), ctx->N, ctx->P_g, min_maf, max_missing, keep);
      if (n_kept) *n_kept = kept;
   });
}

extern "C" int fpca_create_snp_subset(fpca_ctx **out, fpca_ctx *src, const uint8_t *keep, int accum)
{
   if (out) *out = nullptr;
   fpca_ctx *c = nullptr;
   int rc = guarded([&] {
      if (!out || !src || !keep)
         throw Error(FPCA_EINVAL, std::string("bad argument to fpca_create_snp_subset (") + (!out ? "out" : !src ? "src" : "keep") + " is NULL)");
      if (src->dense)
         throw Error(FPCA_EINVAL, "fpca_create_snp_subset: the source holds a dense matrix; SNP subsets compact the packed genotypes (fpca_create, "
                                  "fpca_create_from_bed, synthetic)");
      if (src->multi() || (src->rank_known && src->nranks > 1))
         throw Error(FPCA_EINVAL, "fpca_create_snp_subset: the source is one shard of several (a communicator, an all-reduce hook or fpca_set_rank with "
                                  "more than one rank); SNP subsets are made from a single context only");
      const std::vector<uint32_t> idx = kept_indices(keep, src->P_g);
      if (idx.empty())
         throw Error(FPCA_EINVAL, "fpca_create_snp_subset: the mask keeps 0 of " + std::to_string(src->P_g) + " SNPs; at least 1 is needed");
      c = new fpca_ctx();
      try {
         ctx_alloc_common(c, src->N, idx.size(), src->stand, src->device, accum);
      } catch (const Error &e) {
         if (e.code != FPCA_ENOMEM) throw;
         size_t fr = 0, tot = 0;
         (void)hipMemGetInfo(&fr, &tot);
         const double gb = 1.0 / (1024.0 * 1024.0 * 1024.0);
         char msg[512];
         std::snprintf(msg, sizeof(msg),
                       "fpca_create_snp_subset: the subset's packed genotypes need %.2f GiB of device memory (%llu of %llu SNPs x %llu samples at 2 bits) "
                       "beside the source's %.2f GiB, which stays resident until it is destroyed; %.2f of %.2f GiB are free on device %d",
                       (double)(c->pitch * c->P_pad) * gb, (unsigned long long)idx.size(), (unsigned long long)src->P_g, (unsigned long long)src->N,
                       (double)(src->pitch * src->P_pad) * gb, (double)fr * gb, (double)tot * gb, src->device);
         throw Error(FPCA_ENOMEM, msg);
      }
      HIP_CHECK(hipStreamSynchronize(src->stream)); // (nothing writes the source's matrix after its upload; its stream may still read it)
      DevMem<uint32_t> d_idx(idx.size(), "fpca_create_snp_subset", "the list of the kept SNPs");
      HIP_CHECK(hipMemcpyAsync(d_idx.p, idx.data(), idx.size() * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
      kern::gather_records(src->d_packed, src->pitch, d_idx.p, idx.size(), c->d_packed, c->stream); // (behind the 0x55 memset, same stream)
      HIP_CHECK(hipStreamSynchronize(c->stream));
   });
   if (rc != FPCA_OK) {
      if (c) ctx_free(c);
      return rc;
   }
   *out = c;
   return FPCA_OK;
}
