// pcrelate.hpp -- PRIVATE to libfpca.so: the host side that pcrelate.hip (PC-Relate kinship) and pcrelate_ibd.hip (PC-Relate IBD sharing)
// share -- the refusals, the design matrix, the factor and beta, the sample-major copy, the map from a slab's samples to panel rows, the
// test-build switches and the constants of the panel layout.  The definitions are in pcrelate.hip.
#pragma once
#include <cstdint>
#include <vector>

#include "ctx.hpp"

namespace fpca {

constexpr int PCR_TILE = 64;                         // samples per workgroup tile side (2 waves x 32)
constexpr int PCR_STEP = 16;                         // SNPs of one LDS step
constexpr int PCR_CHUNK = 512;                       // panels are whole chunks of this many SNPs
constexpr int PCR_MAXD = 32;                         // columns of V: 1 + npc
constexpr int PCR_BLK_SNPS = 64;                     // SNPs (and samples) of one workgroup of the operand kernels
constexpr uint64_t PCR_BLOCK_LIMIT = 1ull << 30;     // bytes of one output buffer of a block call
constexpr uint64_t PCR_LAUNCH_PAIRS = 1ull << 18;    // tile pairs of one launch
constexpr uint64_t PCR_SLAB_BYTES = 1ull << 28;      // the sums of one slab, all arrays together
constexpr uint64_t PCR_PANEL_BYTES = 1ull << 30;     // the operand panels, all arrays together
constexpr int PCR_RECT = 0, PCR_TRI = 1;

typedef double d4 __attribute__((ext_vector_type(4)));
typedef double d2 __attribute__((ext_vector_type(2)));

// device buffers of one call
struct PcrBufs {
   DevMem<uint8_t> d_smp; // the sample-major copy [N_pad][pitch]
   size_t pitch = 0;
   DevMem<double> d_V, d_beta; // [N][d], [P_g][d]
   DevMem<d2> d_panel;
   uint64_t panel_snps = 0, panel_rows = 0; // SNPs of a panel; the rows it has room for
   DevMem<double> d_S, d_D, d_kin, d_den;   // the slab: sums [rows][ld], outputs
   size_t ld = 0;
   int d = 0;
   double lo = 0, hi = 0;
};

// how the samples of a slab map to panel rows: the row tiles [i0, i0 + 64 nti) and the column tiles [j0, j0 + 64 ntj) as one run of rows
// where they overlap or touch, else one after the other
struct PcrMap {
   uint64_t s0, n0, s1, rows, pa0, pb0;
};

void pcr_refuse(const fpca_ctx *c, const char *fn);
std::vector<double> pcr_design(const fpca_ctx *c, const char *fn, const double *pcs, int npc);
void pcr_factor(const fpca_ctx *c, const char *fn, const std::vector<double> &V, int d, const uint8_t *train, std::vector<double> &lc);
void pcr_beta_dev(fpca_ctx *c, const char *fn, const std::vector<double> &V, int d, const uint8_t *train, const std::vector<double> &lc, double *d_beta);
void pcr_make_operand(fpca_ctx *c, PcrBufs &s, const char *fn, const std::vector<double> &V, int d, const double *beta);
PcrMap pcr_map(uint64_t i0, uint64_t iend, uint64_t j0, uint64_t jend);
// the value of a test-build switch rounded up to `unit`, 0 when it is not set.  Called through PCR_ENV, so that the product holds no name.
uint64_t pcr_env(const char *value, uint64_t unit);
#define PCR_ENV(name, unit) ::fpca::pcr_env(FPCA_TEST_ENV(name), unit)

} // namespace fpca
