// king.hip -- KING-robust kinship and the unrelated-sample cutoff: fpca_king_block / fpca_king_pairs / fpca_king_cutoff (include/fpca.h
// "Kinship"), fpca_debug_king_rule / fpca_bench_king.
//
// The KING-robust estimator (Manichaikul et al. 2010) of a pair of samples is made of sums over the SNPs called in both -- the products
// k_ld_band accumulates per pair of SNPs, with the records being samples and K running along the SNPs: the LD Gram on the transposed
// matrix, over the full triangle instead of a band, with another integer epilogue.  ld_planes.hpp holds the shared loop (without e.e).
//   operand       a row-major sample-major copy of the packed matrix, made for the call (kern::transpose_packed, not band-tiled) and freed
//                 before it returns: N_pad rows of pitch = round_up(P_pad / 4, 128) bytes preset to PAD_BYTE, so the pad SNPs read as
//                 missing on both sides; npad = 4 pitch - P_g.  kern::ld_totals gives (sum x, sum x^2, sum e) per sample over that pitch.
//   k_king        one workgroup (4 waves, 2 x 2) per pair of 64-sample tiles; a wave owns one 32 x 32 block of pairs and FIVE accumulator
//                 planes (x.x, x.e, e.x, q.e, e.q: 80 registers); no LDS, no barrier.  Records past the last are read as the last and
//                 dropped in the epilogue.  A wave whose two 32-sample blocks hold no missing call (sum e == npad) multiplies x.x only.
//                 BLOCK: phi[ni][nj] as fp64 over any rectangle.  PAIRS: the strict upper triangle; (i, j, phi) of every pair with
//                 phi > thr whose samples are both in `keep` is appended to a list through atomicAdd on one counter (a vector-memory
//                 atomic); a slot is stored only below the capacity, the counter keeps counting.
// The cutoff rule runs on the host (king_cutoff_rule): greedy removal by degree with a lazily cleaned heap.
#include <algorithm>
#include <cmath>
#include <limits>
#include <queue>

#include "ctx.hpp"
#include "launch_check.hpp"
#include "ld_planes.hpp"

using namespace fpca;

namespace {

constexpr int KING_TILE = 64;                         // samples per workgroup tile side (2 waves x 32)
constexpr uint64_t KING_MAX_P = 1ull << 28;           // 4 P_pad < 2^31: every sum fits the int32 accumulators
constexpr uint64_t KING_BLOCK_LIMIT = 1ull << 30;     // bytes of an fpca_king_block buffer
constexpr uint64_t KING_LAUNCH_PAIRS = 1ull << 18;    // tile pairs of one launch
constexpr uint64_t KING_CUTOFF_CAP = 1ull << 26;      // pairs fpca_king_cutoff keeps room for
constexpr int KING_BLOCK = 0, KING_PAIRS = 1;

// workgroup w -> (tI, tJ) = (w / ntj, w % ntj): tile tI holds samples [i0 + 64 tI, ...), tile tJ samples [j0 + 64 tJ, ...)
template <int MODE>
__global__ __launch_bounds__(256, 2) void k_king(const uint8_t *__restrict__ packed, size_t pitch, const uint32_t *__restrict__ tot, uint32_t npad,
                                                 uint64_t nrec, uint64_t i0, uint64_t iend, uint64_t j0, uint64_t jend, uint32_t ntj, int force_general,
                                                 double *__restrict__ phi, const uint8_t *__restrict__ keep, double thr, uint64_t cap,
                                                 unsigned long long *__restrict__ count, uint32_t *__restrict__ out_i, uint32_t *__restrict__ out_j,
                                                 double *__restrict__ out_phi)
{
   const uint64_t tI = blockIdx.x / ntj, tJ = blockIdx.x % ntj;
   const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, li = lane & 31, kh = lane >> 5;
   // this wave's 32 x 32 block of pairs: samples ia .. ia + 31 (MFMA operand A, output rows) x ja .. ja + 31 (operand B, output columns)
   const uint64_t ia = i0 + tI * KING_TILE + (uint64_t)(wave >> 1) * 32, ja = j0 + tJ * KING_TILE + (uint64_t)(wave & 1) * 32;
   // nothing to do (wave-uniform; the kernel has no barrier): the block lies past the range, or (PAIRS) wholly on or below the diagonal
   if (ia >= iend || ja >= jend) return;
   if (MODE == KING_PAIRS && ja + 31 <= ia) return;
   // records past the last one are read as the last one (their pairs are dropped in the epilogue): no load leaves [0, nrec)
   const uint64_t ra = ia + li < nrec ? ia + li : nrec - 1, rb = ja + li < nrec ? ja + li : nrec - 1;
   const uint4 ta = reinterpret_cast<const uint4 *>(tot)[ra], tb = reinterpret_cast<const uint4 *>(tot)[rb]; // (sum x, sum x^2, sum e, -)
   const bool general = force_general || __builtin_amdgcn_ballot_w64(ta.z != npad || tb.z != npad) != 0ull;
   const uint4 *pa = reinterpret_cast<const uint4 *>(packed + ra * pitch) + kh * 4;
   const uint4 *pb = reinterpret_cast<const uint4 *>(packed + rb * pitch) + kh * 4;
   const uint32_t nchunks = (uint32_t)(pitch / 128);
   v16i acc[5];
#pragma unroll
   for (int m = 0; m < 5; m++)
#pragma unroll
      for (int r = 0; r < 16; r++) acc[m][r] = 0;
   if (general)
      ld_products<true, false>(pa, pb, nchunks, acc);
   else
      ld_products<false, false>(pa, pb, nchunks, acc); // e is 1 at the pad SNPs of both sides only, where x = q = 0: the mixed products stay 0
   // Epilogue.  The planes hold sums over ALL 4 pitch SNP slots, pad SNPs included, and e = 1 - m, so with the padded totals Sx = sum x,
   // Sq = sum x^2 of a sample and h = 2x - q (1 at a heterozygous call, else 0):
   //    het_i = sum h_i m_j = 2 (Sx_i - x_i.e_j) - (Sq_i - q_i.e_j)        het_j = 2 (Sx_j - e_i.x_j) - (Sq_j - e_i.q_j)
   //    D = sum (x_i - x_j)^2 m_i m_j = (Sq_i - q_i.e_j) + (Sq_j - e_i.q_j) - 2 x_i.x_j          (x = 0 where missing)
   // All of it exact in int64; the quotient is ONE fp64 divide of two converted integers.
   const uint64_t j = ja + li;
   const bool keep_j = MODE == KING_PAIRS && j < jend && (!keep || keep[j]);
#pragma unroll
   for (int r = 0; r < 16; r++) {
      const int row = (r & 3) + 8 * (r >> 2) + 4 * kh; // v_mfma_i32_32x32x32_i8: register r of lane (li, kh) is D[row][li]
      const uint64_t i = ia + row;
      if (i >= iend || j >= jend) continue;
      if (MODE == KING_PAIRS && (j <= i || !keep_j || (keep && !keep[i]))) continue;
      const uint4 ti = reinterpret_cast<const uint4 *>(tot)[i];
      const int64_t qi = (int64_t)ti.y - acc[3][r], qj = (int64_t)tb.y - acc[4][r];
      const int64_t het_i = 2 * ((int64_t)ti.x - acc[1][r]) - qi, het_j = 2 * ((int64_t)tb.x - acc[2][r]) - qj;
      const int64_t D = qi + qj - 2 * (int64_t)acc[0][r], hmin = het_i < het_j ? het_i : het_j;
      const double v = hmin == 0 ? __builtin_nan("") : (double)(2 * hmin - D) / (double)(4 * hmin);
      if (MODE == KING_BLOCK) {
         phi[(size_t)(i - i0) * (jend - j0) + (j - j0)] = v;
      } else if (v > thr) {
         const unsigned long long slot = atomicAdd(count, 1ull);
         if (slot < cap) {
            out_i[slot] = (uint32_t)i;
            out_j[slot] = (uint32_t)j;
            out_phi[slot] = v;
         }
      }
   }
}

// what every entry point refuses (before any device work)
void king_refuse(const fpca_ctx *c, const char *fn)
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
   if (c->P_g > KING_MAX_P)
      throw Error(FPCA_EINVAL, std::string(fn) + ": " + std::to_string(c->P_g) + " SNPs; above 2^28 = 268,435,456 the sums no longer fit 32 bits");
   if (c->N > 0xFFFFFFFFull) throw Error(FPCA_EINVAL, std::string(fn) + ": this context has " + std::to_string(c->N) + " samples; at most 2^32 - 1");
}

bool king_force_general()
{
   const char *v = FPCA_TEST_ENV("FPCA_KING_FORCE_GENERAL");
   return v && *v && *v != '0';
}

// device buffers of one call
struct KingBufs {
   DevMem<uint8_t> d_smp, d_keep; // the sample-major copy [N_pad][pitch]; keep [N]
   size_t pitch = 0;
   uint32_t npad = 0;
   DevMem<uint32_t> d_tot, d_i, d_j;
   DevMem<double> d_phi;
   DevMem<unsigned long long> d_count;
   // the pair list of `slots` entries and its counter
   void alloc_pairs(size_t slots, const char *fn)
   {
      d_i = DevMem<uint32_t>(slots, fn, "the pair list (i)");
      d_j = DevMem<uint32_t>(slots, fn, "the pair list (j)");
      d_phi = DevMem<double>(slots, fn, "the pair list (phi)");
      d_count = DevMem<unsigned long long>(1, fn, "the pair counter");
   }
};

// the sample-major operand and its per-sample totals, enqueued on the context's stream
void king_make_operand(fpca_ctx *c, KingBufs &s, const char *fn)
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

void king_launch(int mode, const fpca_ctx *c, const KingBufs &s, uint64_t i0, uint64_t iend, uint64_t j0, uint64_t jend, double *phi, double thr,
                 uint64_t cap)
{
   const uint64_t nti = (iend - i0 + KING_TILE - 1) / KING_TILE, ntj = (jend - j0 + KING_TILE - 1) / KING_TILE, wgs = nti * ntj;
   if (!wgs) return;
   if (wgs > 0x7FFFFFFFull || ntj > 0xFFFFFFFFull) throw Error(FPCA_EINVAL, "kinship: " + std::to_string(wgs) + " tile pairs exceed one launch");
   if (mode == KING_BLOCK)
      hipLaunchKernelGGL(k_king<KING_BLOCK>, dim3((unsigned)wgs), dim3(256), 0, c->stream, s.d_smp.p, s.pitch, s.d_tot.p, s.npad, c->N, i0, iend, j0, jend,
                         (uint32_t)ntj, (int)king_force_general(), phi, s.d_keep.p, thr, cap, s.d_count.p, s.d_i.p, s.d_j.p, s.d_phi.p);
   else
      hipLaunchKernelGGL(k_king<KING_PAIRS>, dim3((unsigned)wgs), dim3(256), 0, c->stream, s.d_smp.p, s.pitch, s.d_tot.p, s.npad, c->N, i0, iend, j0, jend,
                         (uint32_t)ntj, (int)king_force_general(), phi, s.d_keep.p, thr, cap, s.d_count.p, s.d_i.p, s.d_j.p, s.d_phi.p);
   launch_check();
}

// the strict upper triangle in slabs of row tiles: slab [ta, tb) x column tiles [ta, nt); the blocks below the diagonal return at once
void king_triangle(const fpca_ctx *c, const KingBufs &s, double thr, uint64_t cap)
{
   const uint64_t N = c->N, nt = (N + KING_TILE - 1) / KING_TILE;
   uint64_t forced = 0;
   if (const char *v = FPCA_TEST_ENV("FPCA_KING_SLAB_ROWS"))
      if (std::atoll(v) > 0) forced = ((uint64_t)std::atoll(v) + KING_TILE - 1) / KING_TILE;
   for (uint64_t ta = 0; ta < nt;) {
      const uint64_t rows = forced ? forced : std::max<uint64_t>(KING_LAUNCH_PAIRS / (nt - ta), 1), tb = std::min(ta + rows, nt);
      king_launch(KING_PAIRS, c, s, ta * KING_TILE, std::min(tb * KING_TILE, N), ta * KING_TILE, N, nullptr, thr, cap);
      ta = tb;
   }
}

struct KingPair {
   uint32_t i, j;
   double phi;
};

// the pair pass: every pair i < j of kept samples with phi > thr, sorted by (i, j), when no more than `cap` qualify; returns how many do
uint64_t king_pair_pass(fpca_ctx *c, const char *fn, const uint8_t *keep, double thr, uint64_t cap, std::vector<KingPair> &out)
{
   const uint64_t N = c->N;
   cap = std::min<uint64_t>(cap, N * (N - 1) / 2);
   HIP_CHECK(hipSetDevice(c->device));
   KingBufs s;
   king_make_operand(c, s, fn);
   if (keep) {
      s.d_keep = DevMem<uint8_t>(N, fn, "the sample mask");
      HIP_CHECK(hipMemcpyAsync(s.d_keep.p, keep, N, hipMemcpyHostToDevice, c->stream));
   }
   s.alloc_pairs((size_t)std::max<uint64_t>(cap, 1), fn);
   HIP_CHECK(hipMemsetAsync(s.d_count.p, 0, sizeof(unsigned long long), c->stream));
   king_triangle(c, s, thr, cap);
   unsigned long long found = 0;
   HIP_CHECK(hipMemcpyAsync(&found, s.d_count.p, sizeof(found), hipMemcpyDeviceToHost, c->stream));
   HIP_CHECK(hipStreamSynchronize(c->stream));
   out.clear();
   if (found > cap || found == 0) return found;
   std::vector<uint32_t> hi(found), hj(found);
   std::vector<double> hp(found);
   HIP_CHECK(hipMemcpy(hi.data(), s.d_i.p, found * sizeof(uint32_t), hipMemcpyDeviceToHost));
   HIP_CHECK(hipMemcpy(hj.data(), s.d_j.p, found * sizeof(uint32_t), hipMemcpyDeviceToHost));
   HIP_CHECK(hipMemcpy(hp.data(), s.d_phi.p, found * sizeof(double), hipMemcpyDeviceToHost));
   out.resize(found);
   for (uint64_t k = 0; k < found; k++) out[k] = {hi[k], hj[k], hp[k]};
   std::sort(out.begin(), out.end(), [](const KingPair &a, const KingPair &b) { return a.i != b.i ? a.i < b.i : a.j < b.j; });
   return found;
}

} // namespace

namespace fpca {

uint64_t king_cutoff_rule(const uint32_t *pi, const uint32_t *pj, uint64_t n_pairs, uint64_t N, uint8_t *keep)
{
   for (uint64_t k = 0; k < N; k++) keep[k] = keep[k] ? 1 : 0;
   // the graph on the kept samples: every listed pair once, whatever its order or multiplicity
   std::vector<std::pair<uint32_t, uint32_t>> edges;
   edges.reserve(n_pairs);
   for (uint64_t k = 0; k < n_pairs; k++) {
      const uint32_t a = std::min(pi[k], pj[k]), b = std::max(pi[k], pj[k]);
      if (b >= N) throw Error(FPCA_EINVAL, "kinship cutoff: pair " + std::to_string(k) + " names sample " + std::to_string(b) + " of " + std::to_string(N));
      if (a != b && keep[a] && keep[b]) edges.emplace_back(a, b);
   }
   std::sort(edges.begin(), edges.end());
   edges.erase(std::unique(edges.begin(), edges.end()), edges.end());
   std::vector<uint64_t> ptr(N + 1, 0);
   for (const auto &e : edges) {
      ptr[e.first + 1]++;
      ptr[e.second + 1]++;
   }
   for (uint64_t k = 0; k < N; k++) ptr[k + 1] += ptr[k];
   std::vector<uint32_t> adj(2 * edges.size());
   {
      std::vector<uint64_t> fill(ptr.begin(), ptr.end() - 1);
      for (const auto &e : edges) {
         adj[fill[e.first]++] = e.second;
         adj[fill[e.second]++] = e.first;
      }
   }
   // largest degree first, the largest index among equals; an entry whose degree is no longer current is skipped when it surfaces
   std::vector<uint64_t> deg(N);
   std::priority_queue<std::pair<uint64_t, uint32_t>> heap;
   for (uint64_t k = 0; k < N; k++) {
      deg[k] = ptr[k + 1] - ptr[k];
      if (deg[k]) heap.emplace(deg[k], (uint32_t)k);
   }
   while (!heap.empty()) {
      const auto top = heap.top();
      heap.pop();
      const uint32_t v = top.second;
      if (!keep[v] || top.first != deg[v] || deg[v] == 0) continue;
      keep[v] = 0;
      for (uint64_t a = ptr[v]; a < ptr[v + 1]; a++) {
         const uint32_t u = adj[a];
         if (!keep[u]) continue;
         if (--deg[u]) heap.emplace(deg[u], u);
      }
      deg[v] = 0;
   }
   uint64_t kept = 0;
   for (uint64_t k = 0; k < N; k++) kept += keep[k];
   return kept;
}

} // namespace fpca

extern "C" int fpca_king_block(fpca_ctx *ctx, uint64_t i0, uint64_t ni, uint64_t j0, uint64_t nj, double *phi)
{
   return guarded([&] {
      king_refuse(ctx, "fpca_king_block");
      if (!phi) throw Error(FPCA_EINVAL, "bad argument to fpca_king_block (phi is NULL)");
      const uint64_t N = ctx->N;
      if (ni == 0 || nj == 0 || i0 >= N || ni > N - i0 || j0 >= N || nj > N - j0)
         throw Error(FPCA_EINVAL, "fpca_king_block: samples [" + std::to_string(i0) + ", " + std::to_string(i0) + " + " + std::to_string(ni) + ") x [" +
                                      std::to_string(j0) + ", " + std::to_string(j0) + " + " + std::to_string(nj) +
                                      ") are not a non-empty rectangle of this context's " + std::to_string(N) + " samples");
      if (ni > KING_BLOCK_LIMIT / sizeof(double) / nj)
         throw Error(FPCA_EINVAL, "fpca_king_block: a block of " + std::to_string(ni) + " x " + std::to_string(nj) + " doubles is over the limit of " +
                                      std::to_string(KING_BLOCK_LIMIT) + " bytes; call it block by block");
      const size_t count = (size_t)ni * nj;
      HIP_CHECK(hipSetDevice(ctx->device));
      KingBufs s;
      king_make_operand(ctx, s, "fpca_king_block");
      DevMem<double> d_out(count, "fpca_king_block", "the block of coefficients");
      king_launch(KING_BLOCK, ctx, s, i0, i0 + ni, j0, j0 + nj, d_out.p, 0.0, 0);
      HIP_CHECK(hipMemcpyAsync(phi, d_out.p, count * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
      HIP_CHECK(hipStreamSynchronize(ctx->stream));
   });
}

extern "C" int fpca_king_pairs(fpca_ctx *ctx, const uint8_t *keep, double thr, uint64_t max_pairs, uint32_t *i, uint32_t *j, double *phi,
                               uint64_t *n_pairs)
{
   return guarded([&] {
      king_refuse(ctx, "fpca_king_pairs");
      if (!n_pairs || (max_pairs && (!i || !j || !phi))) throw Error(FPCA_EINVAL, "bad argument to fpca_king_pairs (a NULL output)");
      if (std::isnan(thr)) throw Error(FPCA_EINVAL, "fpca_king_pairs: the threshold is NaN");
      std::vector<KingPair> pairs;
      const uint64_t found = king_pair_pass(ctx, "fpca_king_pairs", keep, thr, max_pairs, pairs);
      *n_pairs = found;
      if (found > max_pairs)
         throw Error(FPCA_ENOMEM, "fpca_king_pairs: " + std::to_string(found) + " pairs are above the threshold, the arrays hold " +
                                      std::to_string(max_pairs) + "; call again with room for " + std::to_string(found));
      for (uint64_t k = 0; k < found; k++) {
         i[k] = pairs[k].i;
         j[k] = pairs[k].j;
         phi[k] = pairs[k].phi;
      }
   });
}

extern "C" int fpca_king_cutoff(fpca_ctx *ctx, double thr, uint8_t *keep, uint64_t *n_kept)
{
   return guarded([&] {
      king_refuse(ctx, "fpca_king_cutoff");
      if (!keep) throw Error(FPCA_EINVAL, "bad argument to fpca_king_cutoff (keep is NULL)");
      if (std::isnan(thr)) throw Error(FPCA_EINVAL, "fpca_king_cutoff: the threshold is NaN");
      uint64_t cap = KING_CUTOFF_CAP;
      if (const char *v = FPCA_TEST_ENV("FPCA_KING_MAX_PAIRS"))
         if (std::atoll(v) > 0) cap = (uint64_t)std::atoll(v);
      std::vector<KingPair> pairs;
      const uint64_t found = king_pair_pass(ctx, "fpca_king_cutoff", keep, thr, cap, pairs);
      if (found > cap)
         throw Error(FPCA_ENOMEM, "fpca_king_cutoff: " + std::to_string(found) + " pairs are above the threshold, the call keeps room for " +
                                      std::to_string(cap) + "; raise the threshold or thin the samples first (fpca_king_pairs lists them)");
      std::vector<uint32_t> pi(found), pj(found);
      for (uint64_t k = 0; k < found; k++) {
         pi[k] = pairs[k].i;
         pj[k] = pairs[k].j;
      }
      const uint64_t kept = king_cutoff_rule(pi.data(), pj.data(), found, ctx->N, keep);
      if (n_kept) *n_kept = kept;
   });
}

extern "C" int fpca_debug_king_rule(const uint32_t *i, const uint32_t *j, uint64_t n_pairs, uint64_t N, uint8_t *keep, uint64_t *n_kept)
{
   return guarded([&] {
      if (!keep || (n_pairs && (!i || !j)) || N > 0xFFFFFFFFull) throw Error(FPCA_EINVAL, "bad argument to fpca_debug_king_rule");
      for (uint64_t k = 0; k < n_pairs; k++)
         if (i[k] >= N || j[k] >= N)
            throw Error(FPCA_EINVAL, "fpca_debug_king_rule: pair " + std::to_string(k) + " is outside the " + std::to_string(N) + " samples");
      const uint64_t kept = king_cutoff_rule(i, j, n_pairs, N, keep);
      if (n_kept) *n_kept = kept;
   });
}

extern "C" int fpca_bench_king(fpca_ctx *ctx, int reps, double *ms, double *macs)
{
   return guarded([&] {
      king_refuse(ctx, "fpca_bench_king");
      if (!ms || reps < 1) throw Error(FPCA_EINVAL, "bad argument to fpca_bench_king");
      HIP_CHECK(hipSetDevice(ctx->device));
      const uint64_t N = ctx->N, cap = 1ull << 20;
      const double thr = 0.0884;
      KingBufs s;
      king_make_operand(ctx, s, "fpca_bench_king");
      s.alloc_pairs(cap, "fpca_bench_king");
      DevEvent e0("fpca_bench_king"), e1("fpca_bench_king");
      HIP_CHECK(hipMemsetAsync(s.d_count.p, 0, sizeof(unsigned long long), ctx->stream));
      king_triangle(ctx, s, thr, cap);
      for (int r = 0; r < reps; r++) {
         HIP_CHECK(hipMemsetAsync(s.d_count.p, 0, sizeof(unsigned long long), ctx->stream));
         HIP_CHECK(hipEventRecord(e0, ctx->stream));
         king_triangle(ctx, s, thr, cap);
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
         const bool force = king_force_general();
         double mfma = 0;
         for (uint64_t bi = 0; bi < nb; bi++)
            for (uint64_t bj = bi; bj < nb; bj++) mfma += (force || !clean[bi] || !clean[bj]) ? 5.0 : 1.0;
         *macs = mfma * (double)(s.pitch / 128) * 16.0 * 32768.0;
      }
   });
}
