// scca.hpp -- PRIVATE to libfpca.so: what scca.hip (fpca_scca_prepare / fpca_scca_fit) shares with scca_cv.hip (fpca_scca_cv): the
// resident cross-product matrix with its workspaces, and the iteration loop that leaves one model on the device.
#pragma once
#include "ctx.hpp"

// what a context keeps between fpca_scca_prepare and fpca_scca_fit (fpca_scca_cv builds one of its own per call)
struct fpca_scca_state {
   int k = 0, kp = 0;
   double invdiv = 1;
   double *d_C = nullptr;       // [P_g][kp]
   std::vector<double> Yh;      // N x k column-major: the standardised phenotypes * invdiv (Py = Yh V is a host product)
   // workspaces of the fits, grown on demand
   double *d_ws = nullptr;
   size_t ws_cap = 0;
   int *d_flags = nullptr; // [0] done (0 running, 1 converged, 2 u vanished, 3 v vanished), [1] iterations completed
   ~fpca_scca_state()
   {
      if (d_C) (void)hipFree(d_C);
      if (d_ws) (void)hipFree(d_ws);
      if (d_flags) (void)hipFree(d_flags);
   }
};

namespace fpca {

// k_scca_v<1024> keeps w and v (2 * k_pad doubles, dynamic) beside its buf [1024] and red [16] (static, 8,320 B by the code object's
// metadata) in LDS: 69,760 B at the maximum, of the 160 KB one workgroup may use on gfx950 (64 KB would stop at k = 3568)
constexpr int SCCA_MAX_K = 3840;
constexpr int SCCA_V_LDS_MAX = 8 * (1024 + 16) + 2 * 8 * SCCA_MAX_K;
static_assert(SCCA_MAX_K % 16 == 0 && SCCA_V_LDS_MAX <= 160 * 1024, "k_scca_v at SCCA_MAX_K does not fit one workgroup's LDS");

// one model as scca_fit_dev leaves it: U [ndim][P_g] and V [ndim][kp] in the state's workspace (valid until the next fit on that
// state), everything of length ndim on the host
struct SccaDevFit {
   double *dU = nullptr, *dV = nullptr;
   std::vector<double> d;
   std::vector<int> iters;
   int converged = 0, status = 0;
};

// the iteration of RandomPCA::scca on st->d_C from V0 (host, k x ndim, leading dimension ldv0) with the edge rules of fpca_scca_fit:
// no download of U, no pass over the genotypes; the stream has finished every iteration when it returns
void scca_fit_dev(fpca_ctx *c, fpca_scca_state *st, double lambda1, double lambda2, int ndim, int maxiter, double tol, const double *V0,
                  int64_t ldv0, SccaDevFit &fit);
// T (where K2 left a chunk, [P_pad][b] row-major) -> columns [c0, min(c0 + b, kp)) of C, scaled; columns >= nc of the chunk are C's zero pad
void scca_store_c(const double *T, uint64_t P_g, int b, int nc, double scale, double *Cm, int kp, int c0, hipStream_t s);
void scca_check_single(const fpca_ctx *c, const char *fn); // FPCA_EINVAL for a context that is one shard of several

} // namespace fpca
