// pcair.hip -- PC-AiR's unrelated set, chosen by KING kinship and ancestry divergence: fpca_king_census / fpca_pcair_partition /
// fpca_pcair_king / fpca_pcair_pairs (include/fpca.h "Kinship"), fpca_bench_king_census.
//
// PC-AiR (Conomos, Miller & Thornton 2015) reads KING-robust phi twice: phi > kin_thr makes a pair RELATED, phi < div_thr makes it
// DIVERGENT in ancestry.  The partition needs the related pairs as a list and, of every sample, the NUMBER of its divergent pairs.  In a
// structured cohort most of the N^2 / 2 pairs are divergent: no list holds them, so they are counted where they are found.
//   operand         king.hip's: a row-major sample-major copy of the packed matrix made for the call and freed before it returns, and the
//                   per-sample totals over it (kern::transpose_packed, kern::ld_totals); this file keeps its own copy of the set-up, as
//                   king_rel.hip does.
//   k_king_census   the geometry and the inner loop of k_king: one workgroup (4 waves, 2 x 2) per pair of 64-sample tiles; a wave owns one
//                   32 x 32 block of pairs and five accumulator planes (ld_planes.hpp); no LDS, no barrier; the clean-block fast path;
//                   the strict upper triangle in slabs of at most 2^18 tile pairs.  phi is formed as in k_king, bit for bit.  The epilogue
//                   classifies a pair (related / divergent / neither), appends the related ones to k_king<PAIRS>'s list when there is
//                   one (cap > 0), and counts both classes per sample: register r of lane (li, kh) is D[(r & 3) + 8 (r >> 2) + 4 kh][li],
//                   so ONE ballot of a predicate holds an output row's 32 columns in each half of the mask -- a popcount and one atomicAdd
//                   per row by lane li == 0 of each half, only when non-zero -- and a lane's own 16 registers count its column: the two
//                   halves are added with a cross-lane move, one atomicAdd per column by the lower half.  A pair i < j is seen once and
//                   credited to i (its row) and j (its column).  Plain vector-memory integer atomics on uint32: exact, so the counts are
//                   the same in any order; no fp atomics.
//   exclusion list  pairs never counted divergent (relatives known from elsewhere): a CSR keyed by the smaller index, rows sorted; a pair is
//                   looked up (binary search in row i) only once it has been found divergent and row i is not empty.
// The partition rule runs on the host (pcair_partition_rule): greedy removal by (degree, n_div, sum of kinship, index) with a lazily cleaned
// heap; memory linear in N + edges.
#include <algorithm>
#include <cmath>
#include <limits>
#include <queue>

#include "ctx.hpp"
#include "launch_check.hpp"
#include "ld_planes.hpp"

using namespace fpca;

namespace {

constexpr int CEN_TILE = 64;                         // samples per workgroup tile side (2 waves x 32)
constexpr uint64_t CEN_MAX_P = 1ull << 28;           // 4 P_pad < 2^31: every sum fits the int32 accumulators
constexpr uint64_t CEN_LAUNCH_PAIRS = 1ull << 18;    // tile pairs of one launch
constexpr uint64_t CEN_PAIR_CAP = 1ull << 26;        // related pairs fpca_pcair_king keeps room for

// what one launch reads and writes beside the operand
struct CensusArgs {
   const uint8_t *keep;          // [N] or null
   double kin_thr, div_thr;
   const uint64_t *excl_ptr;     // [N + 1] or null: row i of excl_adj holds the j > i of the excluded pairs (i, j), ascending
   const uint32_t *excl_adj;
   uint64_t cap;                 // slots of the pair list; 0: no list, the counter is not touched
   unsigned long long *count;
   uint32_t *out_i, *out_j;
   double *out_phi;
   uint32_t *n_rel, *n_div;      // [N], preset to 0
};

// workgroup w -> (tI, tJ) = (w / ntj, w % ntj): tile tI holds samples [i0 + 64 tI, ...), tile tJ samples [j0 + 64 tJ, ...)
__global__ __launch_bounds__(256, 2) void k_king_census(const uint8_t *__restrict__ packed, size_t pitch, const uint32_t *__restrict__ tot,
                                                        uint32_t npad, uint64_t nrec, uint64_t i0, uint64_t iend, uint64_t j0, uint64_t jend,
                                                        uint32_t ntj, int force_general, CensusArgs g)
{
   const uint64_t tI = blockIdx.x / ntj, tJ = blockIdx.x % ntj;
   const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, li = lane & 31, kh = lane >> 5;
   // this wave's 32 x 32 block of pairs: samples ia .. ia + 31 (MFMA operand A, output rows) x ja .. ja + 31 (operand B, output columns)
   const uint64_t ia = i0 + tI * CEN_TILE + (uint64_t)(wave >> 1) * 32, ja = j0 + tJ * CEN_TILE + (uint64_t)(wave & 1) * 32;
   // nothing to do (wave-uniform; the kernel has no barrier): the block lies past the range, or wholly on or below the diagonal
   if (ia >= iend || ja >= jend) return;
   if (ja + 31 <= ia) return;
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
   // Epilogue: het_i, het_j, D and phi exactly as in k_king (king.hip); then the class of the pair and the counts.
   const uint64_t j = ja + li;
   const bool keep_j = j < jend && (!g.keep || g.keep[j]);
   uint32_t col_rel = 0, col_div = 0; // this lane's 16 rows of column j
#pragma unroll
   for (int r = 0; r < 16; r++) {
      const int row = (r & 3) + 8 * (r >> 2) + 4 * kh; // v_mfma_i32_32x32x32_i8: register r of lane (li, kh) is D[row][li]
      const uint64_t i = ia + row;
      bool rel = false, dv = false;
      if (i < iend && j > i && keep_j && (!g.keep || g.keep[i])) {
         const uint4 ti = reinterpret_cast<const uint4 *>(tot)[i];
         const int64_t qi = (int64_t)ti.y - acc[3][r], qj = (int64_t)tb.y - acc[4][r];
         const int64_t het_i = 2 * ((int64_t)ti.x - acc[1][r]) - qi, het_j = 2 * ((int64_t)tb.x - acc[2][r]) - qj;
         const int64_t D = qi + qj - 2 * (int64_t)acc[0][r], hmin = het_i < het_j ? het_i : het_j;
         const double v = hmin == 0 ? __builtin_nan("") : (double)(2 * hmin - D) / (double)(4 * hmin);
         rel = v > g.kin_thr;
         dv = !rel && v < g.div_thr;
         if (dv && g.excl_ptr) { // wave-uniform when there is no list
            uint64_t lo = g.excl_ptr[i], hi = g.excl_ptr[i + 1];
            while (lo < hi) { // the first entry of row i that is >= j
               const uint64_t mid = lo + (hi - lo) / 2;
               if (g.excl_adj[mid] < (uint32_t)j)
                  lo = mid + 1;
               else
                  hi = mid;
            }
            if (lo < g.excl_ptr[i + 1] && g.excl_adj[lo] == (uint32_t)j) dv = false;
         }
         if (rel && g.cap) {
            const unsigned long long slot = atomicAdd(g.count, 1ull);
            if (slot < g.cap) {
               g.out_i[slot] = (uint32_t)i;
               g.out_j[slot] = (uint32_t)j;
               g.out_phi[slot] = v;
            }
         }
      }
      // row i = ia + row of this half of the wave: its 32 columns are this half's 32 bits of the ballot
      const uint32_t row_rel = (uint32_t)__builtin_popcount((uint32_t)(__builtin_amdgcn_ballot_w64(rel) >> (32 * kh)));
      const uint32_t row_div = (uint32_t)__builtin_popcount((uint32_t)(__builtin_amdgcn_ballot_w64(dv) >> (32 * kh)));
      if (li == 0) { // a non-zero count means a pair passed the test above: i < iend
         if (row_rel) atomicAdd(g.n_rel + i, row_rel);
         if (row_div) atomicAdd(g.n_div + i, row_div);
      }
      col_rel += rel;
      col_div += dv;
   }
   // column j: rows 4 kh + {0..3, 8..11, ...} are here, the others in lane li of the other half
   col_rel += (uint32_t)__shfl_xor((int)col_rel, 32);
   col_div += (uint32_t)__shfl_xor((int)col_div, 32);
   if (kh == 0) { // a non-zero count means j < jend
      if (col_rel) atomicAdd(g.n_rel + j, col_rel);
      if (col_div) atomicAdd(g.n_div + j, col_div);
   }
}

// what every entry point refuses (before any device work): the refusals of king.hip, word for word
void cen_refuse(const fpca_ctx *c, const char *fn)
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
   if (c->P_g > CEN_MAX_P)
      throw Error(FPCA_EINVAL, std::string(fn) + ": " + std::to_string(c->P_g) + " SNPs; above 2^28 = 268,435,456 the sums no longer fit 32 bits");
   if (c->N > 0xFFFFFFFFull) throw Error(FPCA_EINVAL, std::string(fn) + ": this context has " + std::to_string(c->N) + " samples; at most 2^32 - 1");
}

void cen_check_thresholds(const char *fn, double kin_thr, double div_thr)
{
   if (std::isnan(kin_thr) || std::isnan(div_thr)) throw Error(FPCA_EINVAL, std::string(fn) + ": a threshold is NaN");
}

bool cen_force_general()
{
   const char *v = FPCA_TEST_ENV("FPCA_KING_FORCE_GENERAL");
   return v && *v && *v != '0';
}

// the exclusion list as the kernel reads it: every pair once as (smaller, larger), rows by the smaller index, each ascending
struct ExclCsr {
   std::vector<uint64_t> ptr;
   std::vector<uint32_t> adj;
};

// FPCA_EINVAL for a pair with i == j or an index >= N; `what` names the list in the message
void check_pairs(const char *fn, const char *what, const uint32_t *pi, const uint32_t *pj, uint64_t n, uint64_t N)
{
   if (n && (!pi || !pj)) throw Error(FPCA_EINVAL, std::string("bad argument to ") + fn + " (" + what + " is NULL)");
   for (uint64_t k = 0; k < n; k++) {
      if (pi[k] >= N || pj[k] >= N)
         throw Error(FPCA_EINVAL, std::string(fn) + ": " + what + " pair " + std::to_string(k) + " names sample " +
                                      std::to_string(std::max(pi[k], pj[k])) + " of " + std::to_string(N));
      if (pi[k] == pj[k])
         throw Error(FPCA_EINVAL, std::string(fn) + ": " + what + " pair " + std::to_string(k) + " pairs sample " + std::to_string(pi[k]) + " with itself");
   }
}

ExclCsr make_excl(const uint32_t *pi, const uint32_t *pj, uint64_t n, uint64_t N)
{
   std::vector<std::pair<uint32_t, uint32_t>> e(n);
   for (uint64_t k = 0; k < n; k++) e[k] = {std::min(pi[k], pj[k]), std::max(pi[k], pj[k])};
   std::sort(e.begin(), e.end());
   e.erase(std::unique(e.begin(), e.end()), e.end());
   ExclCsr x;
   x.ptr.assign(N + 1, 0);
   x.adj.resize(e.size());
   for (const auto &p : e) x.ptr[p.first + 1]++;
   for (uint64_t k = 0; k < N; k++) x.ptr[k + 1] += x.ptr[k];
   for (size_t k = 0; k < e.size(); k++) x.adj[k] = e[k].second; // sorted by (first, second): already row by row
   return x;
}

// device buffers of one call
struct CenBufs {
   DevMem<uint8_t> d_smp, d_keep; // the sample-major copy [N_pad][pitch]; keep [N]
   size_t pitch = 0;
   uint32_t npad = 0;
   DevMem<uint32_t> d_tot, d_i, d_j, d_nrel, d_ndiv, d_adj;
   DevMem<uint64_t> d_ptr;
   DevMem<double> d_phi;
   DevMem<unsigned long long> d_count;
   CensusArgs g{};
};

// the sample-major operand and its per-sample totals, enqueued on the context's stream (as king.hip makes them)
void cen_make_operand(fpca_ctx *c, CenBufs &s, const char *fn)
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

// everything else of a pass: the mask, the exclusion list, the pair list of `cap` slots (none for 0) and the two count arrays
void cen_make_args(fpca_ctx *c, CenBufs &s, const char *fn, const uint8_t *keep, double kin_thr, double div_thr, const ExclCsr *excl, uint64_t cap)
{
   const uint64_t N = c->N;
   s.g.kin_thr = kin_thr;
   s.g.div_thr = div_thr;
   if (keep) {
      s.d_keep = DevMem<uint8_t>(N, fn, "the sample mask");
      HIP_CHECK(hipMemcpyAsync(s.d_keep.p, keep, N, hipMemcpyHostToDevice, c->stream));
      s.g.keep = s.d_keep.p;
   }
   if (excl && !excl->adj.empty()) {
      s.d_ptr = DevMem<uint64_t>(N + 1, fn, "the exclusion list (rows)");
      s.d_adj = DevMem<uint32_t>(excl->adj.size(), fn, "the exclusion list");
      HIP_CHECK(hipMemcpyAsync(s.d_ptr.p, excl->ptr.data(), (N + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, c->stream));
      HIP_CHECK(hipMemcpyAsync(s.d_adj.p, excl->adj.data(), excl->adj.size() * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
      s.g.excl_ptr = s.d_ptr.p;
      s.g.excl_adj = s.d_adj.p;
   }
   if (cap) {
      s.d_i = DevMem<uint32_t>(cap, fn, "the pair list (i)");
      s.d_j = DevMem<uint32_t>(cap, fn, "the pair list (j)");
      s.d_phi = DevMem<double>(cap, fn, "the pair list (phi)");
      s.d_count = DevMem<unsigned long long>(1, fn, "the pair counter");
      s.g.cap = cap;
      s.g.count = s.d_count.p;
      s.g.out_i = s.d_i.p;
      s.g.out_j = s.d_j.p;
      s.g.out_phi = s.d_phi.p;
   }
   s.d_nrel = DevMem<uint32_t>(N, fn, "the related-pair counts");
   s.d_ndiv = DevMem<uint32_t>(N, fn, "the divergent-pair counts");
   s.g.n_rel = s.d_nrel.p;
   s.g.n_div = s.d_ndiv.p;
}

void cen_clear(const fpca_ctx *c, const CenBufs &s)
{
   if (s.g.cap) HIP_CHECK(hipMemsetAsync(s.d_count.p, 0, sizeof(unsigned long long), c->stream));
   HIP_CHECK(hipMemsetAsync(s.d_nrel.p, 0, c->N * sizeof(uint32_t), c->stream));
   HIP_CHECK(hipMemsetAsync(s.d_ndiv.p, 0, c->N * sizeof(uint32_t), c->stream));
}

// the strict upper triangle in slabs of row tiles: slab [ta, tb) x column tiles [ta, nt); the blocks below the diagonal return at once
void cen_triangle(const fpca_ctx *c, const CenBufs &s)
{
   const uint64_t N = c->N, nt = (N + CEN_TILE - 1) / CEN_TILE;
   uint64_t forced = 0;
   if (const char *v = FPCA_TEST_ENV("FPCA_KING_SLAB_ROWS"))
      if (std::atoll(v) > 0) forced = ((uint64_t)std::atoll(v) + CEN_TILE - 1) / CEN_TILE;
   for (uint64_t ta = 0; ta < nt;) {
      const uint64_t rows = forced ? forced : std::max<uint64_t>(CEN_LAUNCH_PAIRS / (nt - ta), 1), tb = std::min(ta + rows, nt);
      const uint64_t i0 = ta * CEN_TILE, iend = std::min(tb * CEN_TILE, N), ntj = nt - ta, wgs = (tb - ta) * ntj;
      if (wgs > 0x7FFFFFFFull || ntj > 0xFFFFFFFFull) throw Error(FPCA_EINVAL, "kinship: " + std::to_string(wgs) + " tile pairs exceed one launch");
      hipLaunchKernelGGL(k_king_census, dim3((unsigned)wgs), dim3(256), 0, c->stream, s.d_smp.p, s.pitch, s.d_tot.p, s.npad, N, i0, iend, i0, N,
                         (uint32_t)ntj, (int)cen_force_general(), s.g);
      launch_check();
      ta = tb;
   }
}

struct CenPair {
   uint32_t i, j;
   double phi;
};

// one pass: n_rel[N] and n_div[N] and, with cap > 0, the related pairs sorted by (i, j) when no more than `cap` qualify; returns how many
// do (0 without a list)
uint64_t census_pass(fpca_ctx *c, const char *fn, const uint8_t *keep, double kin_thr, double div_thr, const ExclCsr *excl, uint64_t cap,
                     uint32_t *n_rel, uint32_t *n_div, std::vector<CenPair> *out)
{
   const uint64_t N = c->N;
   if (cap) cap = std::max<uint64_t>(std::min<uint64_t>(cap, N * (N - 1) / 2), 1);
   HIP_CHECK(hipSetDevice(c->device));
   CenBufs s;
   cen_make_operand(c, s, fn);
   cen_make_args(c, s, fn, keep, kin_thr, div_thr, excl, cap);
   cen_clear(c, s);
   cen_triangle(c, s);
   unsigned long long found = 0;
   if (cap) HIP_CHECK(hipMemcpyAsync(&found, s.d_count.p, sizeof(found), hipMemcpyDeviceToHost, c->stream));
   HIP_CHECK(hipMemcpyAsync(n_rel, s.d_nrel.p, N * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
   HIP_CHECK(hipMemcpyAsync(n_div, s.d_ndiv.p, N * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
   HIP_CHECK(hipStreamSynchronize(c->stream));
   if (!out) return found;
   out->clear();
   if (found > cap || found == 0) return found;
   std::vector<uint32_t> hi(found), hj(found);
   std::vector<double> hp(found);
   HIP_CHECK(hipMemcpy(hi.data(), s.d_i.p, found * sizeof(uint32_t), hipMemcpyDeviceToHost));
   HIP_CHECK(hipMemcpy(hj.data(), s.d_j.p, found * sizeof(uint32_t), hipMemcpyDeviceToHost));
   HIP_CHECK(hipMemcpy(hp.data(), s.d_phi.p, found * sizeof(double), hipMemcpyDeviceToHost));
   out->resize(found);
   for (uint64_t k = 0; k < found; k++) (*out)[k] = {hi[k], hj[k], hp[k]};
   std::sort(out->begin(), out->end(), [](const CenPair &a, const CenPair &b) { return a.i != b.i ? a.i < b.i : a.j < b.j; });
   return found;
}

} // namespace

namespace fpca {

uint64_t pcair_partition_rule(uint64_t N, uint64_t n_pairs, const uint32_t *pi, const uint32_t *pj, const double *kin, const uint32_t *n_div,
                              uint8_t *keep)
{
   for (uint64_t k = 0; k < n_pairs; k++) { // refused before keep is touched
      const uint32_t a = std::min(pi[k], pj[k]), b = std::max(pi[k], pj[k]);
      if (b >= N)
         throw Error(FPCA_EINVAL, "fpca_pcair_partition: pair " + std::to_string(k) + " names sample " + std::to_string(b) + " of " + std::to_string(N));
      if (a == b) throw Error(FPCA_EINVAL, "fpca_pcair_partition: pair " + std::to_string(k) + " pairs sample " + std::to_string(a) + " with itself");
      if (!std::isfinite(kin[k])) throw Error(FPCA_EINVAL, "fpca_pcair_partition: the kinship of pair " + std::to_string(k) + " is not finite");
   }
   for (uint64_t k = 0; k < N; k++) keep[k] = keep[k] ? 1 : 0;
   // the graph on the kept samples: every listed pair once, whatever its order, with the first kinship listed for it
   struct Edge {
      uint32_t a, b;
      uint64_t k;
   };
   std::vector<Edge> edges;
   edges.reserve(n_pairs);
   for (uint64_t k = 0; k < n_pairs; k++) {
      const uint32_t a = std::min(pi[k], pj[k]), b = std::max(pi[k], pj[k]);
      if (keep[a] && keep[b]) edges.push_back({a, b, k});
   }
   std::sort(edges.begin(), edges.end(), [](const Edge &x, const Edge &y) { return x.a != y.a ? x.a < y.a : x.b != y.b ? x.b < y.b : x.k < y.k; });
   edges.erase(std::unique(edges.begin(), edges.end(), [](const Edge &x, const Edge &y) { return x.a == y.a && x.b == y.b; }), edges.end());
   std::vector<uint64_t> ptr(N + 1, 0);
   for (const auto &e : edges) {
      ptr[e.a + 1]++;
      ptr[e.b + 1]++;
   }
   for (uint64_t k = 0; k < N; k++) ptr[k + 1] += ptr[k];
   // the edges are sorted by (a, b): a row receives its smaller neighbours first, then its larger ones, each ascending
   std::vector<uint32_t> adj(2 * edges.size());
   std::vector<double> akin(2 * edges.size());
   {
      std::vector<uint64_t> fill(ptr.begin(), ptr.end() - 1);
      for (const auto &e : edges) {
         adj[fill[e.a]] = e.b;
         akin[fill[e.a]++] = kin[e.k];
         adj[fill[e.b]] = e.a;
         akin[fill[e.b]++] = kin[e.k];
      }
   }
   // An entry is (degree, sample) as the sample stood when it was pushed; one whose degree is no longer current is skipped when it
   // surfaces.  The kinship sum of an entry is formed only when the entry surfaces at the top (then it is pushed back with the sum): among
   // equal (degree, n_div) the entries without a sum come first, so when one WITH a sum surfaces every current rival has its own.
   struct Entry {
      uint64_t deg;
      uint32_t ndiv;
      bool summed;
      double sum;
      uint32_t v;
   };
   auto below = [](const Entry &x, const Entry &y) { // x goes after y
      if (x.deg != y.deg) return x.deg < y.deg;
      if (x.ndiv != y.ndiv) return x.ndiv > y.ndiv;
      if (x.summed != y.summed) return x.summed;
      if (x.summed && x.sum != y.sum) return x.sum > y.sum;
      return x.v < y.v;
   };
   std::priority_queue<Entry, std::vector<Entry>, decltype(below)> heap(below);
   std::vector<uint64_t> deg(N);
   for (uint64_t k = 0; k < N; k++) {
      deg[k] = ptr[k + 1] - ptr[k];
      if (deg[k]) heap.push({deg[k], n_div[k], false, 0.0, (uint32_t)k});
   }
   while (!heap.empty()) {
      Entry top = heap.top();
      heap.pop();
      const uint32_t v = top.v;
      if (!keep[v] || top.deg != deg[v] || deg[v] == 0) continue;
      if (!top.summed) {
         double sum = 0.0;
         for (uint64_t a = ptr[v]; a < ptr[v + 1]; a++)
            if (keep[adj[a]]) sum += akin[a];
         top.summed = true;
         top.sum = sum;
         heap.push(top);
         continue;
      }
      keep[v] = 0;
      for (uint64_t a = ptr[v]; a < ptr[v + 1]; a++) {
         const uint32_t u = adj[a];
         if (!keep[u]) continue;
         if (--deg[u]) heap.push({deg[u], n_div[u], false, 0.0, u});
      }
      deg[v] = 0;
   }
   uint64_t kept = 0;
   for (uint64_t k = 0; k < N; k++) kept += keep[k];
   return kept;
}

} // namespace fpca

extern "C" int fpca_king_census(fpca_ctx *ctx, const uint8_t *keep, double kin_thr, double div_thr, const uint32_t *excl_i, const uint32_t *excl_j,
                                uint64_t n_excl, uint32_t *n_rel, uint32_t *n_div)
{
   return guarded([&] {
      cen_refuse(ctx, "fpca_king_census");
      if (!n_rel || !n_div) throw Error(FPCA_EINVAL, "bad argument to fpca_king_census (a NULL output)");
      cen_check_thresholds("fpca_king_census", kin_thr, div_thr);
      check_pairs("fpca_king_census", "the exclusion list", excl_i, excl_j, n_excl, ctx->N);
      ExclCsr excl;
      if (n_excl) excl = make_excl(excl_i, excl_j, n_excl, ctx->N);
      census_pass(ctx, "fpca_king_census", keep, kin_thr, div_thr, n_excl ? &excl : nullptr, 0, n_rel, n_div, nullptr);
   });
}

extern "C" int fpca_pcair_partition(uint64_t N, uint64_t n_pairs, const uint32_t *i, const uint32_t *j, const double *kin, const uint32_t *n_div,
                                    uint8_t *keep, uint64_t *n_kept)
{
   return guarded([&] {
      if (N > 0xFFFFFFFFull || (N && (!keep || !n_div)) || (n_pairs && (!i || !j || !kin)))
         throw Error(FPCA_EINVAL, "bad argument to fpca_pcair_partition");
      const uint64_t kept = pcair_partition_rule(N, n_pairs, i, j, kin, n_div, keep);
      if (n_kept) *n_kept = kept;
   });
}

extern "C" int fpca_pcair_king(fpca_ctx *ctx, double kin_thr, double div_thr, uint8_t *keep, uint64_t *n_kept, uint32_t *n_rel, uint32_t *n_div)
{
   return guarded([&] {
      cen_refuse(ctx, "fpca_pcair_king");
      if (!keep) throw Error(FPCA_EINVAL, "bad argument to fpca_pcair_king (keep is NULL)");
      cen_check_thresholds("fpca_pcair_king", kin_thr, div_thr);
      uint64_t cap = CEN_PAIR_CAP;
      if (const char *v = FPCA_TEST_ENV("FPCA_KING_MAX_PAIRS"))
         if (std::atoll(v) > 0) cap = (uint64_t)std::atoll(v);
      const uint64_t N = ctx->N;
      std::vector<uint32_t> rel(N), dv(N);
      std::vector<CenPair> pairs;
      const uint64_t found = census_pass(ctx, "fpca_pcair_king", keep, kin_thr, div_thr, nullptr, cap, rel.data(), dv.data(), &pairs);
      if (found > cap)
         throw Error(FPCA_ENOMEM, "fpca_pcair_king: " + std::to_string(found) + " pairs are above the threshold, the call keeps room for " +
                                      std::to_string(cap) + "; raise the threshold or thin the samples first (fpca_king_pairs lists them)");
      std::vector<uint32_t> pi(found), pj(found);
      std::vector<double> pk(found);
      for (uint64_t k = 0; k < found; k++) {
         pi[k] = pairs[k].i;
         pj[k] = pairs[k].j;
         pk[k] = pairs[k].phi;
      }
      const uint64_t kept = pcair_partition_rule(N, found, pi.data(), pj.data(), pk.data(), dv.data(), keep);
      if (n_kept) *n_kept = kept;
      if (n_rel) std::copy(rel.begin(), rel.end(), n_rel);
      if (n_div) std::copy(dv.begin(), dv.end(), n_div);
   });
}

extern "C" int fpca_pcair_pairs(fpca_ctx *ctx, double div_thr, uint64_t n_pairs, const uint32_t *i, const uint32_t *j, const double *kin,
                                uint8_t *keep, uint64_t *n_kept, uint32_t *n_div)
{
   return guarded([&] {
      cen_refuse(ctx, "fpca_pcair_pairs");
      if (!keep) throw Error(FPCA_EINVAL, "bad argument to fpca_pcair_pairs (keep is NULL)");
      if (n_pairs && !kin) throw Error(FPCA_EINVAL, "bad argument to fpca_pcair_pairs (kin is NULL)");
      cen_check_thresholds("fpca_pcair_pairs", 0.0, div_thr);
      const uint64_t N = ctx->N;
      check_pairs("fpca_pcair_pairs", "the kinship list", i, j, n_pairs, N);
      for (uint64_t k = 0; k < n_pairs; k++)
         if (!std::isfinite(kin[k])) throw Error(FPCA_EINVAL, "fpca_pcair_pairs: the kinship of pair " + std::to_string(k) + " is not finite");
      ExclCsr excl;
      if (n_pairs) excl = make_excl(i, j, n_pairs, N);
      std::vector<uint32_t> rel(N), dv(N);
      census_pass(ctx, "fpca_pcair_pairs", keep, std::numeric_limits<double>::infinity(), div_thr, n_pairs ? &excl : nullptr, 0, rel.data(), dv.data(),
                  nullptr);
      const uint64_t kept = pcair_partition_rule(N, n_pairs, i, j, kin, dv.data(), keep);
      if (n_kept) *n_kept = kept;
      if (n_div) std::copy(dv.begin(), dv.end(), n_div);
   });
}

extern "C" int fpca_bench_king_census(fpca_ctx *ctx, int reps, double *ms)
{
   return guarded([&] {
      cen_refuse(ctx, "fpca_bench_king_census");
      if (!ms || reps < 1) throw Error(FPCA_EINVAL, "bad argument to fpca_bench_king_census");
      HIP_CHECK(hipSetDevice(ctx->device));
      const double thr = std::exp2(-5.5);
      CenBufs s;
      cen_make_operand(ctx, s, "fpca_bench_king_census");
      cen_make_args(ctx, s, "fpca_bench_king_census", nullptr, thr, -thr, nullptr, 1ull << 20);
      DevEvent e0("fpca_bench_king_census"), e1("fpca_bench_king_census");
      cen_clear(ctx, s);
      cen_triangle(ctx, s);
      for (int r = 0; r < reps; r++) {
         cen_clear(ctx, s);
         HIP_CHECK(hipEventRecord(e0, ctx->stream));
         cen_triangle(ctx, s);
         HIP_CHECK(hipEventRecord(e1, ctx->stream));
         HIP_CHECK(hipEventSynchronize(e1));
         ms[r] = elapsed_ms(e0, e1);
      }
   });
}
