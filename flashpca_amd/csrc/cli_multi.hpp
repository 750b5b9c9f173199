// cli_multi.hpp -- the launcher of `flashpca --gpus G`: one process per GPU, each on a contiguous SNP shard of the .bed, around one
// shared memory region (cli_multi.cpp).  main() calls launch -> connect -> [fpca_pca] -> collect, and multi_abort / multi_fail /
// multi_on_exception on the ways out; what the region looks like is this unit's own business.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>

#include "../../include/fpca.h"

struct MultiShared;

struct Multi {
   int ngpus = 1, rank = 0;                // rank 0 is the process that was started; it alone talks and writes the files
   uint64_t snp_begin = 0, snp_count = 0;  // this rank's shard (0, 0 = the whole file)
   double *U = nullptr, *Px = nullptr;     // N x k each, column-major, in the shared region: every rank writes its own rows
   bool test_transport = false;            // FPCA_CLI_TEST_TRANSPORT=shm (test builds): all ranks on one device, sums through host memory
   bool test_collectives = false;          // ... with all-gather / reduce-scatter of its own (shm2)
   // the launcher's own (cli_multi.cpp); main() reads only what is above this line
   MultiShared *sh = nullptr;
   double *V = nullptr, *meansd = nullptr; // P x k and P x 2, column-major, in the shared region
   double *slots = nullptr;                // test transport only: G x slot_cap doubles
   size_t slot_cap = 0;
};

// Maps the shared region, installs rank 0's SIGCHLD / SIGALRM handlers and forks ngpus - 1 children; returns in every process
// with m.rank and its shard set, children silent on stdout.  Nothing may have touched HIP, no thread may be running, before it.
void multi_launch(Multi &m, int ngpus, uint64_t N, uint64_t P_file, int n_dim);
// Opens this rank's shard on `device` and joins the transport: RCCL, or the host-memory test transport.  false: multi_abort().
bool multi_connect(Multi &m, fpca_ctx **ctx, const char *bed_file, uint64_t N, int stand_method, int device, int accum, uint64_t *nsnps);
// Deposits this shard's rows of the loadings (Vloc, may be null) and mean/sd; the children leave here; rank 0 waits for them
// and copies all nsnps rows out to V (if Vloc) and meansd.  false: multi_abort().
bool multi_collect(Multi &m, fpca_ctx *ctx, int n_dim, uint64_t nsnps, const double *Vloc, const double *msloc, double *V, double *meansd);
// a rank that cannot go on says so in the shared region (the first message wins); everybody leaves at the next rendezvous
void multi_fail(Multi &m, const std::string &why);
// after a failed rendezvous: a child exits; rank 0 winds the children down, reports the message and returns EXIT_FAILURE
int multi_abort(Multi &m, fpca_ctx *ctx);
// an exception reached main(): a child marks the run failed and exits; rank 0 winds its children down (nothing without --gpus)
void multi_on_exception();
