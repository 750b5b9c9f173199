// bench_hooks.hip -- include/fpca_debug.h: measurement hooks (HIP-event timing of the operator's stages) and hardware probes.
// Not part of the drop-in boundary.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/fpca_debug.h"
#include "ctx.hpp"
#include "hip_backend.hpp"

using namespace fpca;

extern "C" {

// ---- measurement ---------------------------------------------------------------------------------------
int fpca_bench_apply(fpca_ctx *ctx, int b, int steps, int warmup, fpca_bench_result *res)
{
   return guarded([&] {
      if (!ctx || !res || steps < 1 || warmup < 0) throw Error(FPCA_EINVAL, "bad argument to fpca_bench_apply");
      if (b != 16 && b != 32 && b != 48 && b != 64) throw Error(FPCA_EINVAL, "b must be 16, 32, 48 or 64");
      HIP_CHECK(hipSetDevice(ctx->device));
      ensure_stats(ctx);
      static const char *FN = "fpca_bench_apply";
      DevMem<double> dB((size_t)ctx->N_pad * b, FN, "the input block"), dY((size_t)ctx->N_pad * b, FN, "the output block");
      kern::fill_random(dB.p, ctx->N, ctx->N_pad, b, 12345, ctx->stream);
      std::vector<DevEvent> own; // per step: stage boundaries [0..3], K2 / K3 GEMM kernel [4,5] / [6,7]
      std::vector<hipEvent_t> ev; // (the handles in a row, as apply_xxt_dev takes them)
      own.reserve((size_t)steps * 8);
      for (size_t i = 0; i < (size_t)steps * 8; i++) {
         own.emplace_back(FN);
         ev.push_back(own.back());
      }
      for (int i = 0; i < warmup; i++) apply_xxt_dev(ctx, dB.p, b, dY.p, ctx->stream, nullptr);
      HIP_CHECK(hipStreamSynchronize(ctx->stream));
      for (int i = 0; i < steps; i++) apply_xxt_dev(ctx, dB.p, b, dY.p, ctx->stream, &ev[(size_t)i * 8]);
      HIP_CHECK(hipStreamSynchronize(ctx->stream));
      double t2 = 0, t3 = 0, ta = 0, g2 = 0, g3 = 0;
      for (int i = 0; i < steps; i++) {
         t2 += elapsed_ms(ev[i * 8 + 0], ev[i * 8 + 1]);
         t3 += elapsed_ms(ev[i * 8 + 1], ev[i * 8 + 2]);
         ta += elapsed_ms(ev[i * 8 + 2], ev[i * 8 + 3]);
         g2 += elapsed_ms(ev[i * 8 + 4], ev[i * 8 + 5]);
         g3 += elapsed_ms(ev[i * 8 + 6], ev[i * 8 + 7]);
      }
      res->ms_total = elapsed_ms(ev[0], ev[(size_t)(steps - 1) * 8 + 3]);
      res->ms_xt = t2 / steps;
      res->ms_x = t3 / steps;
      res->ms_allreduce = ta / steps;
      res->ms_gemm_xt = g2 / steps;
      res->ms_gemm_x = g3 / steps;
      res->flops_per_step = 4.0 * (double)ctx->N * (double)ctx->P_g * b;
      res->packed_bytes_per_step = 2.0 * (double)ctx->np * (double)ctx->P_g;
   });
}

int fpca_profile_begin(fpca_ctx *ctx, int max_steps)
{
   return guarded([&] {
      if (!ctx || max_steps < 1) throw Error(FPCA_EINVAL, "bad argument to fpca_profile_begin");
      HIP_CHECK(hipSetDevice(ctx->device));
      while (ctx->prof_ev.size() < (size_t)max_steps * 8) {
         hipEvent_t e;
         HIP_CHECK(hipEventCreate(&e));
         ctx->prof_ev.push_back(e);
      }
      ctx->prof_used = 0;
      ctx->prof_calls = 0;
      ctx->prof_on = true;
   });
}

int fpca_profile_sample_every(fpca_ctx *ctx, int stride)
{
   return guarded([&] {
      if (!ctx || stride < 1) throw Error(FPCA_EINVAL, "bad argument to fpca_profile_sample_every");
      ctx->prof_stride = stride;
   });
}

int fpca_profile_end(fpca_ctx *ctx, int b, fpca_bench_result *res, int *nsteps)
{
   return guarded([&] {
      if (!ctx || !res) throw Error(FPCA_EINVAL, "bad argument to fpca_profile_end");
      HIP_CHECK(hipSetDevice(ctx->device));
      ctx->prof_on = false;
      HIP_CHECK(hipDeviceSynchronize());
      const int n = ctx->prof_used;
      double t2 = 0, t3 = 0, ta = 0, tt = 0, g2 = 0, g3 = 0;
      float ms = 0;
      for (int i = 0; i < n; i++) {
         hipEvent_t *e = &ctx->prof_ev[(size_t)i * 8];
         HIP_CHECK(hipEventElapsedTime(&ms, e[4], e[5]));
         g2 += ms;
         HIP_CHECK(hipEventElapsedTime(&ms, e[6], e[7]));
         g3 += ms;
         HIP_CHECK(hipEventElapsedTime(&ms, e[0], e[1]));
         t2 += ms;
         HIP_CHECK(hipEventElapsedTime(&ms, e[1], e[2]));
         t3 += ms;
         HIP_CHECK(hipEventElapsedTime(&ms, e[2], e[3]));
         ta += ms;
         HIP_CHECK(hipEventElapsedTime(&ms, e[0], e[3]));
         tt += ms;
      }
      std::memset(res, 0, sizeof(*res));
      if (n > 0) {
         res->ms_total = tt;
         res->ms_xt = t2 / n;
         res->ms_x = t3 / n;
         res->ms_allreduce = ta / n;
         res->ms_gemm_xt = g2 / n;
         res->ms_gemm_x = g3 / n;
      }
      res->flops_per_step = 4.0 * (double)ctx->N * (double)ctx->P_g * b;
      res->packed_bytes_per_step = 2.0 * (double)ctx->np * (double)ctx->P_g;
      if (nsteps) *nsteps = n;
   });
}

int fpca_bench_stats(fpca_ctx *ctx, int reps, double *ms_per_launch, double *bytes_per_launch)
{
   return guarded([&] {
      if (!ctx || reps < 1) throw Error(FPCA_EINVAL, "bad argument to fpca_bench_stats");
      HIP_CHECK(hipSetDevice(ctx->device));
      const float ms = time_launches(ctx->stream, "fpca_bench_stats", 1, reps, [&] {
         kern::bed_stats(ctx->d_packed, ctx->pitch, ctx->N, ctx->P_g, ctx->stand, ctx->d_lut, ctx->d_mean, ctx->d_sd, ctx->d_sumsq, nullptr, ctx->stream);
      });
      if (ms_per_launch) *ms_per_launch = ms;
      if (bytes_per_launch) *bytes_per_launch = (double)ctx->np * (double)ctx->P_g;
   });
}

int fpca_debug_snp_qc_rule(const double *mean, const uint32_t *n_missing, uint64_t N, uint64_t P, double min_maf, double max_missing,
                           uint8_t *keep, uint64_t *n_kept)
{
   return guarded([&] {
      if (!mean || !n_missing || !keep || N == 0) throw Error(FPCA_EINVAL, "bad argument to fpca_debug_snp_qc_rule");
      snp_qc_check_thresholds("fpca_debug_snp_qc_rule", min_maf, max_missing);
      const uint64_t kept = snp_qc_rule(mean, n_missing, N, P, min_maf, max_missing, keep);
      if (n_kept) *n_kept = kept;
   });
}

int fpca_debug_snp_subset_bench(fpca_ctx *src, const uint8_t *keep, int reps, double *ms_per_launch, double *bytes_per_launch)
{
   return guarded([&] {
      static const char *FN = "fpca_debug_snp_subset_bench";
      if (!src || !keep || reps < 1 || src->dense) throw Error(FPCA_EINVAL, "bad argument to fpca_debug_snp_subset_bench");
      const std::vector<uint32_t> idx = kept_indices(keep, src->P_g);
      if (idx.empty()) throw Error(FPCA_EINVAL, "fpca_debug_snp_subset_bench: the mask keeps no SNP");
      HIP_CHECK(hipSetDevice(src->device));
      DevMem<uint8_t> d_dst(src->pitch * idx.size(), FN, "the compacted records");
      DevMem<uint32_t> d_idx(idx.size(), FN, "the list of the kept SNPs");
      HIP_CHECK(hipMemcpy(d_idx.p, idx.data(), idx.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
      const float ms = time_launches(src->stream, FN, 1, reps, [&] { kern::gather_records(src->d_packed, src->pitch, d_idx.p, idx.size(), d_dst.p, src->stream); });
      if (ms_per_launch) *ms_per_launch = ms;
      if (bytes_per_launch) *bytes_per_launch = 2.0 * (double)src->pitch * (double)idx.size();
   });
}

// diagnostic used by tests/test_gpu_kernels.py: D = A(16x4) B(4x16) through the MFMA operand mapping of kernels.hip
int fpca_debug_mfma_probe(const double *A, const double *B, double *D)
{
   return guarded([&] {
      static const char *FN = "fpca_debug_mfma_probe";
      DevMem<double> dA(64, FN, "A"), dB(64, FN, "B"), dD(256, FN, "D");
      HIP_CHECK(hipMemcpy(dA.p, A, 64 * sizeof(double), hipMemcpyHostToDevice));
      HIP_CHECK(hipMemcpy(dB.p, B, 64 * sizeof(double), hipMemcpyHostToDevice));
      kern::mfma_layout_probe(dA.p, dB.p, dD.p, nullptr);
      HIP_CHECK(hipDeviceSynchronize());
      HIP_CHECK(hipMemcpy(D, dD.p, 256 * sizeof(double), hipMemcpyDeviceToHost));
   });
}

int fpca_debug_mfma_i8_probe(const int8_t *A, const int8_t *Bt, int32_t *D)
{
   return guarded([&] {
      static const char *FN = "fpca_debug_mfma_i8_probe";
      DevMem<int8_t> dA(1024, FN, "A"), dB(1024, FN, "Bt");
      DevMem<int> dD(1024, FN, "D");
      HIP_CHECK(hipMemcpy(dA.p, A, 1024, hipMemcpyHostToDevice));
      HIP_CHECK(hipMemcpy(dB.p, Bt, 1024, hipMemcpyHostToDevice));
      kern::mfma_i8_probe(dA.p, dB.p, dD.p, nullptr);
      HIP_CHECK(hipDeviceSynchronize());
      HIP_CHECK(hipMemcpy(D, dD.p, 1024 * sizeof(int), hipMemcpyDeviceToHost));
   });
}

int fpca_debug_mfma_i8_ports(int shape, int exchanged, const int8_t *A, const int8_t *Bt, int32_t *D)
{
   return guarded([&] {
      static const char *FN = "fpca_debug_mfma_i8_ports";
      if ((shape != 32 && shape != 16) || !A || !Bt || !D) throw Error(FPCA_EINVAL, "bad argument to fpca_debug_mfma_i8_ports");
      const size_t nd = (size_t)shape * shape;
      DevMem<int8_t> dA(1024, FN, "A"), dB(1024, FN, "Bt");
      DevMem<int> dD(nd, FN, "D");
      HIP_CHECK(hipMemcpy(dA.p, A, 1024, hipMemcpyHostToDevice));
      HIP_CHECK(hipMemcpy(dB.p, Bt, 1024, hipMemcpyHostToDevice));
      kern::mfma_i8_ports(shape, exchanged != 0, dA.p, dB.p, dD.p, nullptr);
      HIP_CHECK(hipDeviceSynchronize());
      HIP_CHECK(hipMemcpy(D, dD.p, nd * sizeof(int), hipMemcpyDeviceToHost));
   });
}

// The K4 hooks start by filling the context's split-K partial buffer (at the size earlier calls left it) with NaNs (all bits set): a
// partial plane that a kernel fails to write then shows in the result instead of reading as a zero of fresh memory -- from the
// second call of a kind on a context on, once the buffer has its size.
static void poison_partials(fpca_ctx *ctx)
{
   if (ctx->be_gpart) HIP_CHECK(hipMemsetAsync(ctx->be_gpart, 0xFF, ctx->be_gpart_cap * sizeof(double), ctx->stream));
}

int fpca_debug_k4(fpca_ctx *ctx, int b, int nq, const double *V, const double *W, double *C_gram, const double *C_in, int use_init,
                  double *Out, double *G_out)
{
   return guarded([&] {
      if (!ctx || !V || !W || nq < 1 || nq > 1000 || (b != 16 && b != 32 && b != 48 && b != 64)) throw Error(FPCA_EINVAL, "bad argument to fpca_debug_k4");
      if ((Out || G_out) && !C_in) throw Error(FPCA_EINVAL, "fpca_debug_k4: Out needs C_in");
      HIP_CHECK(hipSetDevice(ctx->device));
      poison_partials(ctx);
      HipBackend be(ctx, b);
      const int64_t N = (int64_t)ctx->N;
      std::vector<int> hv(nq);
      for (int q = 0; q < nq; q++) {
         hv[q] = be.alloc_block();
         be.upload(hv[q], b, V + (size_t)q * b * N, N);
      }
      const int hw = be.alloc_block();
      be.upload(hw, b, W, N);
      if (C_gram) be.gram(hv.data(), nq, hw, C_gram);
      if (Out || G_out) {
         const int ho = be.alloc_block();
         // (a block out of the context's pool may still hold the output of an earlier, identical call: NaNs, so that a row tile the
         // kernel does not store cannot pass for one it did)
         if (!be.sharded()) HIP_CHECK(hipMemsetAsync(be.full_ptr(ho), 0xFF, (size_t)ctx->N_pad * b * sizeof(double), ctx->stream));
         if (G_out) // the update and the Gram matrix of its output from one launch (HipBackend::gemm_gram)
            be.gemm_gram(hv.data(), nq, C_in, use_init ? hw : -1, ho, G_out);
         else
            be.gemm(hv.data(), nq, C_in, use_init ? hw : -1, ho);
         if (Out) be.download(ho, b, Out, N);
         be.free_block(ho);
      }
      be.free_block(hw);
      for (int h : hv) be.free_block(h);
   });
}

// HipBackend::gemm_gramvw through the backend object the solver drives: Out = W + sum_q V_q C_in[q], Cg[q] = V_q' Out (q < nq), Cg[nq] = Out' Out
int fpca_debug_k4_fused(fpca_ctx *ctx, int b, int nq, const double *V, const double *W, const double *C_in, double *Out, double *Cg)
{
   return guarded([&] {
      if (!ctx || !V || !W || !C_in || !Cg || nq < 1 || nq > 1000 || (b != 16 && b != 32 && b != 48 && b != 64)) throw Error(FPCA_EINVAL, "bad argument to fpca_debug_k4_fused");
      HIP_CHECK(hipSetDevice(ctx->device));
      poison_partials(ctx);
      HipBackend be(ctx, b);
      const int64_t N = (int64_t)ctx->N;
      std::vector<int> hv(nq);
      for (int q = 0; q < nq; q++) {
         hv[q] = be.alloc_block();
         be.upload(hv[q], b, V + (size_t)q * b * N, N);
      }
      const int hw = be.alloc_block();
      be.upload(hw, b, W, N);
      be.gemm_gramvw(hv.data(), nq, C_in, hw, hw, Cg); // (in place, as the solver calls it)
      if (Out) be.download(hw, b, Out, N);
      be.free_block(hw);
      for (int h : hv) be.free_block(h);
   });
}

// HipBackend::gemm / gemm_gram with the output block among the operands, the way solver.cpp calls them:
//   mode 0: gemm(V, nq, C_in, init = W, out = W);  mode 1: gemm(V, nq, C_in, -1, out = V_{nq-1});  mode 2: gemm_gram of mode 1
int fpca_debug_k4_inplace(fpca_ctx *ctx, int b, int nq, const double *V, const double *W, const double *C_in, int mode, double *Out, double *G_out)
{
   return guarded([&] {
      if (!ctx || !V || !C_in || !Out || nq < 1 || nq > 1000 || (b != 16 && b != 32 && b != 48 && b != 64) || mode < 0 || mode > 2)
         throw Error(FPCA_EINVAL, "bad argument to fpca_debug_k4_inplace");
      if (mode == 0 && !W) throw Error(FPCA_EINVAL, "fpca_debug_k4_inplace: mode 0 needs W");
      if ((mode == 2) != (G_out != nullptr)) throw Error(FPCA_EINVAL, "fpca_debug_k4_inplace: G_out goes with mode 2");
      HIP_CHECK(hipSetDevice(ctx->device));
      poison_partials(ctx);
      HipBackend be(ctx, b);
      const int64_t N = (int64_t)ctx->N;
      std::vector<int> hv(nq);
      for (int q = 0; q < nq; q++) {
         hv[q] = be.alloc_block();
         be.upload(hv[q], b, V + (size_t)q * b * N, N);
      }
      int ho = hv[nq - 1];
      if (mode == 0) {
         ho = be.alloc_block();
         be.upload(ho, b, W, N);
         be.gemm(hv.data(), nq, C_in, ho, ho);
      } else if (mode == 1)
         be.gemm(hv.data(), nq, C_in, -1, ho);
      else
         be.gemm_gram(hv.data(), nq, C_in, -1, ho, G_out);
      be.download(ho, b, Out, N); // (the block that was overwritten)
      if (mode == 0) be.free_block(ho);
      for (int h : hv) be.free_block(h);
   });
}

// launch time of the fused update + Gram (kernel + plane reduction) against the two launches it replaces, nq random blocks
int fpca_debug_k4_fused_bench(fpca_ctx *ctx, int b, int nq, int reps, double *ms_fused)
{
   return guarded([&] {
      if (!ctx || nq < 1 || nq > 64 || reps < 1 || !ms_fused) throw Error(FPCA_EINVAL, "bad argument to fpca_debug_k4_fused_bench");
      HIP_CHECK(hipSetDevice(ctx->device));
      const uint64_t rows = ctx->N_pad;
      const int planes = kern::update_gram_planes(rows, nq, b);
      if (!planes) throw Error(FPCA_EINVAL, "no fused update + Gram kernel for this shape");
      static const char *FN = "fpca_debug_k4_fused_bench";
      hipStream_t s = ctx->stream;
      std::vector<DevMem<double>> own;
      std::vector<double *> blk; // (the pointers in a row, as the kernels take them)
      for (int q = 0; q < nq + 1; q++) {
         own.emplace_back(rows * b, FN, "a basis block");
         blk.push_back(own.back().p);
         kern::fill_random(blk[q], ctx->N, rows, b, 100 + q, s);
      }
      DevMem<const double *> d_ptrs(nq + 1, FN, "the block pointers");
      HIP_CHECK(hipMemcpyAsync(d_ptrs.p, blk.data(), (nq + 1) * sizeof(double *), hipMemcpyHostToDevice, s));
      const size_t cnt = (size_t)nq * b * b, cntg = (size_t)(nq + 1) * b * b;
      DevMem<double> d_C(cnt, FN, "the coefficients"), d_part(cntg * (planes + 1), FN, "the partial planes");
      HIP_CHECK(hipMemsetAsync(d_C.p, 0, cnt * sizeof(double), s)); // (zero coefficients: the block stays bounded over the repetitions)
      *ms_fused = time_launches(s, FN, 2, reps, [&] {
         kern::update_gram(d_ptrs.p, nq, d_C.p, blk[nq], blk[nq], rows, b, d_part.p + cntg, s);
         kern::reduce_sum(d_part.p + cntg, d_part.p, cntg, planes, s);
      });
   });
}

int fpca_debug_k4_bench(fpca_ctx *ctx, int b, int nq, int reps, double *ms_gram, double *ms_gemm)
{
   return guarded([&] {
      if (!ctx || nq < 1 || nq > 64 || reps < 1 || (b != 16 && b != 32 && b != 48 && b != 64)) throw Error(FPCA_EINVAL, "bad argument to fpca_debug_k4_bench");
      HIP_CHECK(hipSetDevice(ctx->device));
      const uint64_t rows = ctx->N_pad;
      static const char *FN = "fpca_debug_k4_bench";
      hipStream_t s = ctx->stream;
      std::vector<DevMem<double>> own;
      std::vector<double *> blk; // (the pointers in a row, as the kernels take them)
      for (int q = 0; q < nq + 2; q++) {
         own.emplace_back(rows * b, FN, "a basis block");
         blk.push_back(own.back().p);
         kern::fill_random(blk[q], ctx->N, rows, b, 100 + q, s);
      }
      DevMem<const double *> d_ptrs(nq + 2, FN, "the block pointers");
      HIP_CHECK(hipMemcpyAsync(d_ptrs.p, blk.data(), (nq + 2) * sizeof(double *), hipMemcpyHostToDevice, s));
      const size_t cnt = (size_t)nq * b * b;
      const int grows = kern::gram_rows(rows, nq, b), ns = kern::gram_splits(rows, grows) * 4;
      DevMem<double> d_C(cnt, FN, "the coefficients"), d_G(cnt, FN, "the Gram matrices"), d_part(cnt * ns, FN, "the partial planes");
      kern::fill_random(d_C.p, cnt / b, cnt / b, b, 7, s);
      DevEvent e0(FN), e1(FN), e2(FN);
      for (int w = 0; w < 2; w++) { // warm-up
         kern::gram(d_ptrs.p, nq, blk[nq], d_part.p, rows, b, grows, s);
         kern::reduce_sum(d_part.p, d_G.p, cnt, ns, s);
         kern::block_gemm(d_ptrs.p, nq, d_C.p, blk[nq], blk[nq + 1], rows, b, s);
      }
      HIP_CHECK(hipEventRecord(e0, s));
      for (int r = 0; r < reps; r++) {
         kern::gram(d_ptrs.p, nq, blk[nq], d_part.p, rows, b, grows, s);
         kern::reduce_sum(d_part.p, d_G.p, cnt, ns, s);
      }
      HIP_CHECK(hipEventRecord(e1, s));
      for (int r = 0; r < reps; r++) kern::block_gemm(d_ptrs.p, nq, d_C.p, blk[nq], blk[nq + 1], rows, b, s);
      HIP_CHECK(hipEventRecord(e2, s));
      HIP_CHECK(hipEventSynchronize(e2));
      if (ms_gram) *ms_gram = elapsed_ms(e0, e1) / reps;
      if (ms_gemm) *ms_gemm = elapsed_ms(e1, e2) / reps;
   });
}

// The split-K plans of the fp64 / fp32 / dense kernels, from the helpers the launches themselves use (operator.hip fp_k2_splits /
// fp_k3_splits, kernels.hip *_chunks): nothing is launched.
int fpca_debug_fp_plan(fpca_ctx *ctx, int b, int out[6])
{
   return guarded([&] {
      if (!ctx || !out || b < 1 || b > MAX_BLOCKVEC) throw Error(FPCA_EINVAL, "bad argument to fpca_debug_fp_plan");
      const int bw = pad16(b);
      const bool fp32 = ctx->accum == FPCA_ACCUM_FP32;
      const int s2 = fp_k2_splits(ctx, bw), s3 = fp_k3_splits(ctx, bw);
      const kern::SplitChunks c2 = ctx->dense ? kern::xt_b_dense_chunks(ctx->N_pad, s2) : kern::xt_b_chunks(ctx->N_pad, bw, s2);
      const kern::SplitChunks c3 = ctx->dense ? kern::x_t_dense_chunks(ctx->P_pad, s3) : kern::x_t_chunks(ctx->P_pad, bw, s3, fp32);
      out[0] = s2, out[1] = c2.per_split, out[2] = c2.total;
      out[3] = s3, out[4] = c3.per_split, out[5] = c3.total;
   });
}

// NaNs (all bits set) into the operator's split-K partial buffer and into T, at the sizes earlier calls left them: a partial plane or
// a tile of T that the next product fails to write then shows in its result instead of reading as the previous call's value.
int fpca_debug_poison_partials(fpca_ctx *ctx)
{
   return guarded([&] {
      if (!ctx) throw Error(FPCA_EINVAL, "bad argument to fpca_debug_poison_partials");
      HIP_CHECK(hipSetDevice(ctx->device));
      if (ctx->d_part) HIP_CHECK(hipMemsetAsync(ctx->d_part, 0xFF, ctx->part_cap * sizeof(double), ctx->stream));
      if (ctx->d_T) HIP_CHECK(hipMemsetAsync(ctx->d_T, 0xFF, ctx->T_cap * sizeof(double), ctx->stream));
   });
}

// The index lists of the missing calls as the operator's list routes use them: built, if they are not there yet, by the call the
// operator itself makes (sparse_or_dense for the route i8_mode returns), then downloaded.
int fpca_debug_missing_lists(fpca_ctx *ctx, int b, int by_sample, uint32_t *ptr_out, uint32_t *idx_out, uint64_t idx_cap, uint64_t *nnz)
{
   return guarded([&] {
      if (!ctx || !nnz || (b != 16 && b != 32 && b != 64)) throw Error(FPCA_EINVAL, "bad argument to fpca_debug_missing_lists");
      HIP_CHECK(hipSetDevice(ctx->device));
      ensure_stats(ctx);
      if (!ctx->i8_S || !ensure_i8(ctx, b)) throw Error(FPCA_EINVAL, "fpca_debug_missing_lists: the context does not run the exact-integer arithmetic");
      int mode = i8_mode(ctx, b);
      if (mode == I8M_SPARSE || mode == I8M_HYBRID) mode = sparse_or_dense(ctx, b, mode);
      if (mode != I8M_SPARSE && mode != I8M_HYBRID) throw Error(FPCA_EINVAL, "fpca_debug_missing_lists: the context is not on a route with index lists");
      const uint32_t *d_ptr = by_sample ? ctx->d_smp_ptr : ctx->d_snp_ptr, *d_idx = by_sample ? ctx->d_smp_idx : ctx->d_snp_idx;
      if (!d_ptr || !d_idx) throw Error(FPCA_EINVAL, "fpca_debug_missing_lists: the context holds no lists by sample");
      const uint64_t nrec = by_sample ? ctx->N : ctx->P_g;
      *nnz = ctx->hyb_view ? ctx->hyb_sparse_nnz : ctx->n_missing;
      if (idx_out && idx_cap < *nnz) throw Error(FPCA_EINVAL, "fpca_debug_missing_lists: idx_out is too small (*nnz holds the length)");
      HIP_CHECK(hipStreamSynchronize(ctx->stream));
      if (ptr_out) HIP_CHECK(hipMemcpy(ptr_out, d_ptr, (nrec + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost));
      if (idx_out && *nnz) HIP_CHECK(hipMemcpy(idx_out, d_idx, *nnz * sizeof(uint32_t), hipMemcpyDeviceToHost));
   });
}

// kern::sparse_rows_sum / sparse_rows_sum_f32 on caller data, launched with the arguments the operator passes
int fpca_debug_gather(int b, int use_f32, const uint32_t *ptr, const uint32_t *idx, uint64_t nnz, const void *V, uint64_t v_rows, const double *rowscale,
                      const double *colw, const double *init, uint64_t nrec, uint64_t rows_out, int short_lists, double avg_len, double *out, int *variant)
{
   return guarded([&] {
      std::vector<DevMem<uint8_t>> dev;
      auto upload = [&](const void *h, size_t bytes) -> void * { // (at least 16 bytes: the kernels are handed a pointer for an empty array too)
         dev.emplace_back(bytes, "fpca_debug_gather", "an operand", 16);
         if (h && bytes) HIP_CHECK(hipMemcpy(dev.back().p, h, bytes, hipMemcpyHostToDevice));
         return dev.back().p;
      };
      if ((b != 16 && b != 32 && b != 64) || !ptr || !idx || !V || !out || !variant || v_rows == 0 || v_rows >= (1ull << 32) || rows_out == 0 ||
          nrec > rows_out || rows_out >= (1ull << 31) || nnz >= (1ull << 32))
         throw Error(FPCA_EINVAL, "bad argument to fpca_debug_gather");
      if (use_f32 ? (!colw || rowscale) : (colw != nullptr))
         throw Error(FPCA_EINVAL, "fpca_debug_gather: fp32 rows take colw and no rowscale, fp64 rows no colw");
      // every index the kernels will follow is checked here: they read ptr[0 .. nrec], idx[ptr[r] .. ptr[r + 1]) and the rows idx names
      if (ptr[0] != 0 || ptr[nrec] != nnz) throw Error(FPCA_EINVAL, "fpca_debug_gather: ptr must run from 0 to nnz");
      for (uint64_t r = 0; r < nrec; r++)
         if (ptr[r + 1] < ptr[r]) throw Error(FPCA_EINVAL, "fpca_debug_gather: ptr must not decrease");
      for (uint64_t t = 0; t < nnz; t++)
         if (idx[t] >= v_rows) throw Error(FPCA_EINVAL, "fpca_debug_gather: an index is outside V");
      const size_t esz = use_f32 ? sizeof(float) : sizeof(double), out_bytes = (size_t)rows_out * b * sizeof(double);
      const uint32_t *d_ptr = static_cast<const uint32_t *>(upload(ptr, (nrec + 1) * sizeof(uint32_t)));
      const uint32_t *d_idx = static_cast<const uint32_t *>(upload(idx, nnz * sizeof(uint32_t)));
      const void *d_V = upload(V, (size_t)v_rows * b * esz);
      const double *d_rs = rowscale ? static_cast<const double *>(upload(rowscale, v_rows * sizeof(double))) : nullptr;
      const double *d_cw = colw ? static_cast<const double *>(upload(colw, b * sizeof(double))) : nullptr;
      const double *d_init = init ? static_cast<const double *>(upload(init, out_bytes)) : nullptr;
      double *d_out = static_cast<double *>(upload(nullptr, out_bytes));
      HIP_CHECK(hipMemset(d_out, 0xFF, out_bytes)); // NaNs: a row the kernel does not write cannot pass for a zero
      *variant = kern::sparse_rows_sum_variant(b, rowscale != nullptr, short_lists != 0, avg_len);
      if (use_f32)
         kern::sparse_rows_sum_f32(d_ptr, d_idx, static_cast<const float *>(d_V), d_cw, b, nrec, rows_out, d_out, nullptr, d_init, short_lists != 0, avg_len);
      else
         kern::sparse_rows_sum(d_ptr, d_idx, static_cast<const double *>(d_V), d_rs, b, nrec, rows_out, d_out, nullptr, d_init, short_lists != 0, avg_len);
      HIP_CHECK(hipDeviceSynchronize());
      HIP_CHECK(hipMemcpy(out, d_out, out_bytes, hipMemcpyDeviceToHost));
   });
}

// The slicing kernels of the exact-integer arithmetic on caller data, through the launchers the operator calls (kern::i8_colmax ...
// i8_dequant_rows) and in its order: route 0 = xt_i8 / x_i8's own slicing, route 1 = exchange_slices + the unpacking of apply_sharded.
// Everything a kernel should write is poisoned first; every argument is checked before the device is touched.
int fpca_debug_i8_nsc_pad(int S, int b, int *nsc_pad)
{
   return guarded([&] {
      if (b != 16 && b != 32 && b != 48 && b != 64) throw Error(FPCA_EINVAL, "fpca_debug_i8_nsc_pad: b must be 16, 32, 48 or 64");
      if (S < 2 || S > 8) throw Error(FPCA_EINVAL, "fpca_debug_i8_nsc_pad: S must be 2 .. 8");
      if (!nsc_pad) throw Error(FPCA_EINVAL, "fpca_debug_i8_nsc_pad: nsc_pad is NULL");
      *nsc_pad = kern::gemm_i8_nsc_pad(S, b);
   });
}

int fpca_debug_i8_instances(int32_t *keys, int cap, int *count)
{
   return guarded([&] {
      if (!count) throw Error(FPCA_EINVAL, "fpca_debug_i8_instances: count is NULL");
      if (cap < 0 || (cap > 0 && !keys)) throw Error(FPCA_EINVAL, "fpca_debug_i8_instances: keys is NULL or cap negative");
      static_assert(sizeof(int32_t) == sizeof(int), "the keys travel as int");
      *count = kern::gemm_i8_instances(reinterpret_cast<int(*)[6]>(keys), cap);
   });
}

int fpca_debug_gather_blocks(int gemm_waves, int gemm_vgprs, int gemm_lds, int gather_vgprs, int ncu, uint64_t rows_out, uint32_t *limit,
                             uint32_t *grid_side, uint32_t *grid_inline)
{
   return guarded([&] {
      if (!limit || !grid_side || !grid_inline) throw Error(FPCA_EINVAL, "fpca_debug_gather_blocks: an output is NULL");
      if (gemm_waves < 1 || gemm_waves > 16 || gemm_vgprs < 1 || gemm_vgprs > 512 || gather_vgprs < 1 || gather_vgprs > 512 || gemm_lds < 0 ||
          gemm_lds > 160 * 1024 || ncu < 1 || ncu > 4096 || rows_out < 1)
         throw Error(FPCA_EINVAL, "bad argument to fpca_debug_gather_blocks");
      *limit = kern::gather_blocks_beside(kern::CuFootprint{gemm_waves, gemm_vgprs, gemm_lds}, gather_vgprs, ncu);
      *grid_side = kern::sparse_rows_sum_grid(rows_out, *limit);
      *grid_inline = kern::sparse_rows_sum_grid(rows_out, 0);
   });
}

int fpca_debug_i8_slices(int route, int b, int S, uint64_t rows, uint64_t rows_pad, uint64_t rows_valid, const double *V, const double *rowscale0,
                         const double *rowscale1, const double *peers, int n_peers, fpca_debug_slices_out *out0, fpca_debug_slices_out *out1,
                         int *nsc_pad)
{
   return guarded([&] {
      static const char *FN = "fpca_debug_i8_slices";
      auto bad = [&](const char *what) { throw Error(FPCA_EINVAL, std::string(FN) + ": " + what); };
      if (route != 0 && route != 1) bad("route must be 0 (the operator's slicing) or 1 (the exchange)");
      if (b != 16 && b != 32 && b != 48 && b != 64) bad("b must be 16, 32, 48 or 64");
      if (S < 2 || S > 8) bad("S must be 2 .. 8");
      if (rows_pad < 16 || rows_pad % 16 || rows_pad > (1ull << 20)) bad("rows_pad must be a multiple of 16 from 16 to 2^20");
      if (rows > rows_pad) bad("rows is larger than rows_pad");
      if (rows_valid > rows_pad) bad("rows_valid is larger than rows_pad");
      if (!V) bad("V is NULL");
      if (!out0) bad("out0 is NULL");
      if (rowscale1 && !rowscale0) bad("rowscale1 is given without rowscale0");
      if ((rowscale1 != nullptr) != (out1 != nullptr)) bad("out1 goes with rowscale1: the second operand");
      const int nops = rowscale1 ? 2 : 1;
      if (route == 1 && nops == 2) bad("rowscale1: the exchange (route 1) has one operand");
      if (route == 1 && S * b > 512) bad("S b is larger than 512 on the exchange (route 1)");
      if (n_peers < 0 || n_peers > 63 || (n_peers > 0) != (peers != nullptr)) bad("n_peers must be 0 .. 63 and go with peers");
      if (n_peers && nops == 2) bad("peers go with one operand");
      fpca_debug_slices_out *outs[2] = {out0, out1};
      for (int o = 0; o < nops; o++) {
         const fpca_debug_slices_out &w = *outs[o];
         if (w.copy32 && w.copy64) bad("copy32 and copy64 of one operand: the operator asks for one of them");
         if ((w.copy32 || w.dq32) && S > 4) bad("copy32 / dq32 need S <= 4: fp32 rows hold the 30 bits of four slices and no more");
         if (route == 0 && (w.Qrm || w.dq32 || w.dq64)) bad("Qrm, dq32 and dq64 belong to the exchange (route 1)");
      }
      const double *rs[2] = {rowscale0, rowscale1};
      for (uint64_t t = 0; t < rows * (uint64_t)b; t++)
         if (!std::isfinite(V[t])) bad("V holds a non-finite entry");
      for (int o = 0; o < nops; o++)
         for (uint64_t r = 0; rs[o] && r < rows; r++)
            if (!std::isfinite(rs[o][r])) bad(o ? "rowscale1 holds a non-finite entry" : "rowscale0 holds a non-finite entry");
      for (int t = 0; t < n_peers * 64; t++)
         if (!std::isfinite(peers[t]) || peers[t] < 0.0) bad("peers holds an entry that is not a finite maximum of magnitudes");

      const int nsc = kern::gemm_i8_nsc_pad(S, b), SB = S * b, G = 1 + n_peers;
      if (nsc_pad) *nsc_pad = nsc;
      const size_t n_v = (size_t)rows_pad * b, n_max = 64 * kern::I8_SHARDS, n_cs = (size_t)kern::I8_CS_STRIDE * kern::I8_SHARDS;
      auto nan_fill = [](void *p, size_t bytes) { HIP_CHECK(hipMemset(p, 0xFF, bytes)); }; // all bits set: a NaN in either width

      DevMem<double> dV(n_v, FN, "the operand block"), dAll((size_t)G * 64, FN, "the gathered maxima");
      HIP_CHECK(hipMemset(dV.p, 0, n_v * sizeof(double))); // rows >= rows are zero, as in the operator's blocks
      if (rows) HIP_CHECK(hipMemcpy(dV.p, V, (size_t)rows * b * sizeof(double), hipMemcpyHostToDevice));
      HIP_CHECK(hipMemset(dAll.p, 0xFF, (size_t)G * 64 * sizeof(double)));
      if (n_peers) HIP_CHECK(hipMemcpy(dAll.p + 64, peers, (size_t)n_peers * 64 * sizeof(double), hipMemcpyHostToDevice));
      DevMem<int8_t> dQrm(route == 1 ? (size_t)rows_pad * SB : 0, FN, "the row-major slices");
      if (dQrm.p) HIP_CHECK(hipMemset(dQrm.p, 0x55, (size_t)rows_pad * SB));

      struct Dev { // one operand's buffers
         DevMem<double> rs, colw, c64, q64;
         DevMem<unsigned long long> maxbits;
         DevMem<int8_t> Q;
         DevMem<long long> colsum;
         DevMem<float> c32, q32;
      } dev[2];
      kern::SliceOp ops[2];
      std::vector<unsigned long long> own_bits[2];
      for (int o = 0; o < nops; o++) {
         Dev &d = dev[o];
         const fpca_debug_slices_out &w = *outs[o];
         if (rs[o]) {
            d.rs = DevMem<double>(rows_pad, FN, "a row scale");
            HIP_CHECK(hipMemset(d.rs.p, 0, rows_pad * sizeof(double)));
            if (rows) HIP_CHECK(hipMemcpy(d.rs.p, rs[o], rows * sizeof(double), hipMemcpyHostToDevice));
         }
         d.maxbits = DevMem<unsigned long long>(n_max, FN, "the column maxima");
         d.Q = DevMem<int8_t>((size_t)nsc * rows_pad, FN, "the slices");
         d.colw = DevMem<double>(nsc, FN, "the weights");
         d.colsum = DevMem<long long>(n_cs, FN, "the column sums");
         HIP_CHECK(hipMemset(d.maxbits.p, 0, n_max * sizeof(unsigned long long))); // (zeroed once per apply, as the operator does)
         HIP_CHECK(hipMemset(d.colsum.p, 0, n_cs * sizeof(long long)));
         HIP_CHECK(hipMemset(d.Q.p, 0x55, (size_t)nsc * rows_pad));
         nan_fill(d.colw.p, nsc * sizeof(double));
         if (w.copy32) d.c32 = DevMem<float>(n_v, FN, "the fp32 copy");
         if (w.copy64) d.c64 = DevMem<double>(n_v, FN, "the fp64 copy");
         if (w.dq32) d.q32 = DevMem<float>(n_v, FN, "the fp32 rows");
         if (w.dq64) d.q64 = DevMem<double>(n_v, FN, "the fp64 rows");
         if (d.c32.p) nan_fill(d.c32.p, n_v * sizeof(float));
         if (d.c64.p) nan_fill(d.c64.p, n_v * sizeof(double));
         if (d.q32.p) nan_fill(d.q32.p, n_v * sizeof(float));
         if (d.q64.p) nan_fill(d.q64.p, n_v * sizeof(double));
         // route 1 hands the copies to i8_unpack_slices itself, as apply_sharded's callers do: the SliceOp carries none
         ops[o] = kern::SliceOp{d.rs.p, d.maxbits.p, d.Q.p, d.colw.p, w.colsum ? d.colsum.p : nullptr, route == 0 ? d.c64.p : nullptr,
                                route == 0 ? d.c32.p : nullptr};
      }

      hipStream_t s = nullptr;
      kern::i8_colmax(dV.p, route == 0 ? rows : rows_pad, b, nops, ops, s);
      HIP_CHECK(hipDeviceSynchronize());
      for (int o = 0; o < nops; o++) {
         own_bits[o].resize(n_max);
         HIP_CHECK(hipMemcpy(own_bits[o].data(), ops[o].maxbits, n_max * sizeof(unsigned long long), hipMemcpyDeviceToHost));
      }
      if (nops == 1) kern::i8_maxbits_fold(ops[0].maxbits, dAll.p, s); // the hook's own answer is row 0 of the gathered maxima
      if (route == 1 || n_peers) kern::i8_maxbits_set(dAll.p, G, ops[0].maxbits, s);
      if (route == 0)
         kern::i8_slice(dV.p, rows_pad, rows, b, S, nops, ops, s);
      else {
         kern::i8_slice_rows(dV.p, rows_pad, b, S, ops[0], dQrm.p, s);
         kern::i8_unpack_slices(dQrm.p, rows_pad, b, S, ops[0], s, rows_valid, dev[0].c32.p, dev[0].c64.p);
         if (dev[0].q32.p) kern::i8_dequant_rows(dQrm.p, rows_pad, b, S, ops[0], dev[0].q32.p, nullptr, s);
         if (dev[0].q64.p) kern::i8_dequant_rows(dQrm.p, rows_pad, b, S, ops[0], nullptr, dev[0].q64.p, s);
      }
      HIP_CHECK(hipDeviceSynchronize());

      for (int o = 0; o < nops; o++) {
         const fpca_debug_slices_out &w = *outs[o];
         const Dev &d = dev[o];
         auto down = [&](void *h, const void *p, size_t bytes) {
            if (h) HIP_CHECK(hipMemcpy(h, p, bytes, hipMemcpyDeviceToHost));
         };
         if (w.colmax) {
            if (nops == 1)
               down(w.colmax, dAll.p, 64 * sizeof(double));
            else // (two operands: no launch of the fold; the same maximum over the shards, of the words downloaded above)
               for (int c = 0; c < 64; c++) {
                  unsigned long long m = 0;
                  for (int k = 0; k < kern::I8_SHARDS; k++) m = std::max(m, own_bits[o][k * 64 + c]);
                  std::memcpy(&w.colmax[c], &m, sizeof(double));
               }
         }
         if (w.maxbits_own) std::memcpy(w.maxbits_own, own_bits[o].data(), n_max * sizeof(unsigned long long));
         down(w.maxbits, d.maxbits.p, n_max * sizeof(unsigned long long));
         down(w.Q, d.Q.p, (size_t)nsc * rows_pad);
         down(w.Qrm, dQrm.p, (size_t)rows_pad * SB);
         down(w.colw, d.colw.p, nsc * sizeof(double));
         down(w.colsum, d.colsum.p, n_cs * sizeof(long long));
         down(w.copy32, d.c32.p, n_v * sizeof(float));
         down(w.copy64, d.c64.p, n_v * sizeof(double));
         down(w.dq32, d.q32.p, n_v * sizeof(float));
         down(w.dq64, d.q64.p, n_v * sizeof(double));
      }
   });
}

// dev_scratch.hpp's counters and countdown: they exist in the test build only
int fpca_debug_scratch_live(uint64_t out[3])
{
   return guarded([&] {
#ifdef FPCA_TEST_HOOKS
      if (!out) throw Error(FPCA_EINVAL, "bad argument to fpca_debug_scratch_live");
      for (int k = 0; k < 3; k++) out[k] = g_scratch_live[k].load();
#else
      (void)out;
      throw Error(FPCA_EINVAL, "fpca_debug_scratch_live: this is the product build; the counters exist with -DFPCA_TEST_HOOKS only");
#endif
   });
}

int fpca_debug_scratch_fail_at(uint64_t n)
{
   return guarded([&] {
#ifdef FPCA_TEST_HOOKS
      g_scratch_fail_at.store(n);
#else
      (void)n;
      throw Error(FPCA_EINVAL, "fpca_debug_scratch_fail_at: this is the product build; nothing is injected without -DFPCA_TEST_HOOKS");
#endif
   });
}

// the slice count of the next passes: the field HipBackend::set_cheap sets around the eigensolver's cheap passes
int fpca_debug_set_pass_slices(fpca_ctx *ctx, int Sc)
{
   return guarded([&] {
#ifdef FPCA_TEST_HOOKS
      if (!ctx) throw Error(FPCA_EINVAL, "fpca_debug_set_pass_slices: ctx is NULL");
      if (ctx->i8_S <= 0 || ctx->i8_k2_only)
         throw Error(FPCA_EINVAL, "fpca_debug_set_pass_slices: the context does not run both products in the exact-integer arithmetic");
      if (Sc != 0 && (Sc < 2 || Sc >= ctx->i8_S_req))
         throw Error(FPCA_EINVAL, "fpca_debug_set_pass_slices: Sc must be 0 or from 2 to one below the context's slice count");
      ctx->i8_Sc = Sc;
#else
      (void)ctx;
      (void)Sc;
      throw Error(FPCA_EINVAL, "fpca_debug_set_pass_slices: this is the product build; no pass changes its slice count without -DFPCA_TEST_HOOKS");
#endif
   });
}

int fpca_debug_mfma_peak(int waves_per_simd, int iters, int pattern, double *tflops)
{
   return guarded([&] {
      if (waves_per_simd < 1 || waves_per_simd > 8 || iters < 10 || pattern < 0 || (pattern > 3 && pattern < 10) || pattern > 17 || !tflops)
         throw Error(FPCA_EINVAL, "bad argument");
      if (pattern >= 10) {
         // v_mfma_i32_32x32x32_i8 (TOP/s): 10 = zero operands, 11 = random operands (the same bytes on both ports and in both sets).
         // Which port pays for the bytes:  12 = A random, B zero;  13 = A zero, B random  (equal sets: nothing changes between
         // instructions);  14 = A genotype bytes, B random;  15 = A random, B genotype bytes  (the two sets of a port seeded
         // differently, A alternating every instruction, B holding one set for two).  What the order costs:  16 = as 14 with A holding
         // and B alternating, the order of k_gemm_i8's main loop;  17 = B holding one set for two: the stream of 14 under its own number
         using kern::I8_FILL_GENO;
         using kern::I8_FILL_RANDOM;
         using kern::I8_FILL_ZERO;
         const uint32_t s0 = 0x1234567u;
         kern::I8PeakFill f{{s0, s0, s0, s0}, {I8_FILL_ZERO, I8_FILL_ZERO, I8_FILL_ZERO, I8_FILL_ZERO}, 0};
         const auto port = [&](int p, uint32_t kind) { f.kind[2 * p] = f.kind[2 * p + 1] = kind; };
         if (pattern == 11) port(0, I8_FILL_RANDOM), port(1, I8_FILL_RANDOM);
         if (pattern == 12) port(0, I8_FILL_RANDOM);
         if (pattern == 13) port(1, I8_FILL_RANDOM);
         if (pattern >= 14) {
            port(0, pattern == 15 ? I8_FILL_RANDOM : I8_FILL_GENO);
            port(1, pattern == 15 ? I8_FILL_GENO : I8_FILL_RANDOM);
            f.seed[1] = 0x2468ace1u, f.seed[2] = 0x9abcdef3u, f.seed[3] = 0x5f3759dfu;
            f.order = pattern == 16 ? 1 : 0;
         }
         *tflops = kern::mfma_i8_peak_tops(waves_per_simd, iters, f, nullptr);
      } else
         *tflops = kern::mfma_peak_tflops(waves_per_simd, iters, pattern, nullptr);
   });
}

} // extern "C"
