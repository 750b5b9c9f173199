// cli_multi.cpp -- `flashpca --gpus G`: one process per GPU.
// The parent parses the command line and the .fam/.bim, maps one shared region, and forks G - 1 children BEFORE anything
// touches HIP; every process (the parent is rank 0) opens its contiguous SNP shard of the .bed on its own device, joins
// the RCCL communicator (id made by rank 0, handed over through the shared region) and runs the same fpca_pca -- the host
// algebra is replicated and deterministic, the only data-path exchange is the all-reduce inside the block apply
// (DESIGN section 5).  Eigenvectors / eigenvalues are identical on every rank; the loadings and mean/sd rows of each shard
// are deposited in the shared region and rank 0 writes every file.
#include "cli_multi.hpp"

#include <atomic>
#include <cerrno>
#include <csignal>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <new>
#include <stdexcept>
#include <vector>

#include <sched.h>
#include <sys/mman.h>
#include <sys/prctl.h>
#include <sys/wait.h>
#include <unistd.h>

#include <hip/hip_runtime_api.h>

#include "cli_options.hpp"
#include "common.hpp"

static_assert(std::atomic<int>::is_always_lock_free, "the SIGCHLD handler touches these atomics: they must be lock-free");
struct MultiShared {
   std::atomic<int> failed, id_ready, bar_count, bar_sense;
   std::atomic<int> op_kind[64];             // test transport: the call every rank is in (shm_same_call)
   std::atomic<unsigned long long> op_count[64];
   uint8_t id[FPCA_UNIQUE_ID_BYTES];
   char msg[512];
};

// set in the children of a --gpus run: an exception there must not fall through to rank 0's output code
static int g_child_rank = 0;
static MultiShared *g_shared = nullptr;

// rank 0's view of its children.  A child that dies on its own (segfault, OOM kill, an uncaught exit) can never reach the
// next rendezvous, and rank 0 may itself be blocked inside an RCCL collective waiting for it -- so the parent watches
// SIGCHLD: an abnormal child exit that nobody announced in the shared region ends the whole run at once.
static pid_t g_children[64];
static int g_nchildren = 0;
static volatile sig_atomic_t g_child_done[64];
static volatile sig_atomic_t g_quiesce = 0; // set while rank 0 itself winds the children down

static void kill_children()
{
   for (int i = 0; i < g_nchildren; i++)
      if (!g_child_done[i]) (void)kill(g_children[i], SIGKILL);
}

static void on_sigchld(int)
{
   const int saved = errno;
   for (int i = 0; i < g_nchildren; i++) {
      if (g_child_done[i]) continue;
      int st = 0;
      if (waitpid(g_children[i], &st, WNOHANG) != g_children[i]) continue;
      g_child_done[i] = 1;
      const bool bad = WIFSIGNALED(st) || (WIFEXITED(st) && WEXITSTATUS(st) != 0);
      if (bad && !g_quiesce && g_shared && g_shared->failed.load() == 0) {
         g_shared->failed.fetch_add(1);
         static const char msg[] = "Exception: a GPU rank of the --gpus run died unexpectedly\nTerminating\n";
         (void)!write(2, msg, sizeof(msg) - 1);
         kill_children();
         _exit(EXIT_FAILURE);
      }
      // A rank that ANNOUNCED its failure and left: normally everybody meets at the next rendezvous and rank 0 reports the
      // message -- unless the others (rank 0 included) sit inside a collective that the leaver will never join.  Give the
      // orderly path five seconds, then end the run from the alarm.
      if (bad && !g_quiesce) alarm(5);
   }
   errno = saved;
}

static void on_sigalrm(int)
{
   if (g_quiesce) return;
   static const char head[] = "Exception: ";
   static const char tail[] = " (the other ranks were still inside a collective)\nTerminating\n";
   (void)!write(2, head, sizeof(head) - 1);
   if (g_shared) (void)!write(2, g_shared->msg, strnlen(g_shared->msg, sizeof(g_shared->msg)));
   (void)!write(2, tail, sizeof(tail) - 1);
   kill_children();
   _exit(EXIT_FAILURE);
}

// rank 0: wait for every child that has not been reaped yet (the handler may reap them first: ECHILD is fine)
static void wait_children()
{
   for (int i = 0; i < g_nchildren; i++) {
      if (g_child_done[i]) continue;
      (void)waitpid(g_children[i], nullptr, 0);
      g_child_done[i] = 1;
   }
}

// rank 0 cannot go on (exception, early return after the fork): tell the children through the shared region, give them two
// seconds to leave at their next rendezvous, then kill what is left (a child inside an RCCL collective never gets there)
static void abandon_children()
{
   if (g_child_rank > 0 || g_nchildren == 0) return;
   g_quiesce = 1;
   if (g_shared) g_shared->failed.fetch_add(1);
   for (int t = 0; t < 200; t++) {
      bool all = true;
      for (int i = 0; i < g_nchildren; i++) {
         if (g_child_done[i]) continue;
         if (waitpid(g_children[i], nullptr, WNOHANG) != 0) // reaped here, or already by the handler (ECHILD)
            g_child_done[i] = 1;
         else
            all = false;
      }
      if (all) return;
      usleep(10000);
   }
   kill_children();
   wait_children();
}

void multi_fail(Multi &m, const std::string &why)
{
   if (!m.sh) return;
   if (m.sh->failed.fetch_add(1) == 0) std::snprintf(m.sh->msg, sizeof(m.sh->msg), "rank %d: %s", m.rank, why.c_str());
}

// all ranks arrive, or somebody failed (returns false)
static bool multi_barrier(Multi &m)
{
   MultiShared *sh = m.sh;
   const int sense = sh->bar_sense.load();
   if (sh->bar_count.fetch_add(1) + 1 == m.ngpus) {
      sh->bar_count.store(0);
      sh->bar_sense.store(sense ^ 1);
      return sh->failed.load() == 0;
   }
   while (sh->bar_sense.load() == sense) {
      if (sh->failed.load()) return false;
      sched_yield();
   }
   return sh->failed.load() == 0;
}

// Test transport (FPCA_CLI_TEST_TRANSPORT=shm; only in builds with -DFPCA_TEST_HOOKS, i.e. _build/testhooks/flashpca):
// every rank on the SAME device, the sum staged through host shared memory in rank order -- exercises the launcher, the
// sharding and the gather of the outputs on a one-GPU box, where RCCL refuses two ranks on one device.  The shipped CLI
// has no such path: its only transport is RCCL.
#ifdef FPCA_TEST_HOOKS
// the hook contract of fpca.h: a collective fails on every rank or on none.  Every rank announces (call kind, count) before the
// first rendezvous and checks after it that all ranks are in the SAME call -- ranks out of step (one of them took an error path
// the others did not) all see the mismatch and all return non-zero.
static bool shm_same_call(Multi &m, int kind, uint64_t count)
{
   m.sh->op_kind[m.rank].store(kind);
   m.sh->op_count[m.rank].store(count);
   if (!multi_barrier(m)) return false;
   for (int r = 0; r < m.ngpus; r++)
      if (m.sh->op_kind[r].load() != kind || m.sh->op_count[r].load() != count) {
         std::fprintf(stderr, "[fpca-cli] rank %d: the ranks are not in the same collective (rank %d: kind %d count %llu; here kind %d count %llu)\n", m.rank, r,
                      m.sh->op_kind[r].load(), (unsigned long long)m.sh->op_count[r].load(), kind, (unsigned long long)count);
         return false;
      }
   return true;
}
int shm_allreduce(void *user, double *dbuf, uint64_t count, void *stream)
{
   Multi &m = *static_cast<Multi *>(user);
   if (count > m.slot_cap) return -1;
   if (hipStreamSynchronize((hipStream_t)stream) != hipSuccess) return -1;
   if (hipMemcpy(m.slots + (size_t)m.rank * m.slot_cap, dbuf, count * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) return -1;
   if (!shm_same_call(m, 1, count)) return -1;
   std::vector<double> sum(count, 0.0);
   for (int r = 0; r < m.ngpus; r++) {
      const double *p = m.slots + (size_t)r * m.slot_cap;
      for (uint64_t i = 0; i < count; i++) sum[i] += p[i];
   }
   if (!multi_barrier(m)) return -1; // nobody overwrites a slot before everyone has read it
   return hipMemcpy(dbuf, sum.data(), count * sizeof(double), hipMemcpyHostToDevice) == hipSuccess ? 0 : -1;
}
// FPCA_CLI_TEST_TRANSPORT=shm2: all-gather and reduce-scatter of their own as well (fpca_set_collectives), so that the
// row-sharded solver runs the call sequence it runs over RCCL -- per row chunk, on the communication stream -- on one device
int shm_allgather(void *user, const double *send, double *recv, uint64_t count, void *stream)
{
   Multi &m = *static_cast<Multi *>(user);
   if (count > m.slot_cap) return -1;
   if (hipStreamSynchronize((hipStream_t)stream) != hipSuccess) return -1;
   if (hipMemcpy(m.slots + (size_t)m.rank * m.slot_cap, send, count * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) return -1;
   if (!shm_same_call(m, 2, count)) return -1;
   for (int r = 0; r < m.ngpus; r++)
      if (hipMemcpy(recv + (size_t)r * count, m.slots + (size_t)r * m.slot_cap, count * sizeof(double), hipMemcpyHostToDevice) != hipSuccess) return -1;
   return multi_barrier(m) ? 0 : -1;
}
int shm_reducescatter(void *user, const double *send, double *recv, uint64_t count, void *stream)
{
   Multi &m = *static_cast<Multi *>(user);
   if (count * (uint64_t)m.ngpus > m.slot_cap) return -1;
   if (hipStreamSynchronize((hipStream_t)stream) != hipSuccess) return -1;
   if (hipMemcpy(m.slots + (size_t)m.rank * m.slot_cap, send, count * m.ngpus * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) return -1;
   if (!shm_same_call(m, 3, count)) return -1;
   std::vector<double> sum(count, 0.0);
   for (int r = 0; r < m.ngpus; r++) {
      const double *p = m.slots + (size_t)r * m.slot_cap + (size_t)m.rank * count;
      for (uint64_t i = 0; i < count; i++) sum[i] += p[i];
   }
   if (!multi_barrier(m)) return -1;
   return hipMemcpy(recv, sum.data(), count * sizeof(double), hipMemcpyHostToDevice) == hipSuccess ? 0 : -1;
}
#endif

void multi_launch(Multi &mg, int ngpus, uint64_t N, uint64_t P_file, int n_dim)
{
   mg.ngpus = ngpus;
   if (P_file < (uint64_t)ngpus) throw std::runtime_error("fewer SNPs than GPUs");
   const char *tt = FPCA_TEST_ENV("FPCA_CLI_TEST_TRANSPORT");
   mg.test_transport = tt && (std::string(tt) == "shm" || std::string(tt) == "shm2");
   mg.test_collectives = tt && std::string(tt) == "shm2";
   if (mg.test_transport)
      std::cerr << "[fpca-cli] FPCA_CLI_TEST_TRANSPORT=shm: all ranks share one device and exchange through host memory -- a test "
                   "hook for one-GPU boxes, not a way to run" << std::endl;
   mg.slot_cap = mg.test_transport ? (size_t)(N + 1024 + 512 * (size_t)ngpus) * 64 : 0; // the row-sharded solver's padded blocks
   const size_t head = (sizeof(MultiShared) + 63) / 64 * 64;
   const size_t bytes = head + ((size_t)P_file * (n_dim + 2) + 2 * (size_t)N * n_dim + (size_t)ngpus * mg.slot_cap) * sizeof(double);
   void *mem = mmap(nullptr, bytes, PROT_READ | PROT_WRITE, MAP_SHARED | MAP_ANONYMOUS, -1, 0);
   if (mem == MAP_FAILED) throw std::runtime_error(std::string("mmap of the shared region failed: ") + strerror(errno));
   mg.sh = new (mem) MultiShared(); // (fresh anonymous pages: every counter and the message start at zero)
   mg.V = reinterpret_cast<double *>(static_cast<char *>(mem) + head);
   mg.meansd = mg.V + (size_t)P_file * n_dim;
   mg.U = mg.meansd + (size_t)P_file * 2;
   mg.Px = mg.U + (size_t)N * n_dim;
   mg.slots = mg.Px + (size_t)N * n_dim;
   std::cout.flush();
   std::fflush(nullptr);
   g_shared = mg.sh;
   struct sigaction sa;
   std::memset(&sa, 0, sizeof(sa));
   sa.sa_handler = on_sigchld;
   sa.sa_flags = SA_RESTART | SA_NOCLDSTOP;
   sigaction(SIGCHLD, &sa, nullptr);
   sa.sa_handler = on_sigalrm;
   sigaction(SIGALRM, &sa, nullptr);
   const pid_t parent = getpid();
   // SIGCHLD stays blocked until every child pid is registered: a child that dies at once is then still found by the
   // handler (a pending SIGCHLD is delivered on unblocking; the handler polls every registered child)
   sigset_t chld, oldmask;
   sigemptyset(&chld);
   sigaddset(&chld, SIGCHLD);
   sigprocmask(SIG_BLOCK, &chld, &oldmask);
   for (int r = 1; r < ngpus; r++) { // nothing has touched HIP yet: the children initialise their own runtime
      const pid_t pid = fork();
      if (pid < 0) {
         multi_fail(mg, std::string("fork failed: ") + strerror(errno));
         break;
      }
      if (pid == 0) {
         // a child never outlives rank 0 (it may sit in an RCCL collective that will never complete)
         (void)prctl(PR_SET_PDEATHSIG, SIGKILL);
         if (getppid() != parent) _exit(1);
         signal(SIGCHLD, SIG_DFL);
         signal(SIGALRM, SIG_DFL);
         sigprocmask(SIG_SETMASK, &oldmask, nullptr);
         mg.rank = r;
         g_nchildren = 0;
         g_child_rank = r;
         std::cout.setstate(std::ios::failbit); // progress lines come from rank 0 only
         break;
      }
      g_child_done[g_nchildren] = 0;
      g_children[g_nchildren++] = pid;
   }
   if (mg.rank == 0) sigprocmask(SIG_SETMASK, &oldmask, nullptr);
   mg.snp_begin = P_file * (uint64_t)mg.rank / (uint64_t)ngpus;
   mg.snp_count = P_file * (uint64_t)(mg.rank + 1) / (uint64_t)ngpus - mg.snp_begin;
}

int multi_abort(Multi &mg, fpca_ctx *ctx)
{
   if (mg.rank > 0) {
      if (ctx) fpca_destroy(ctx);
      _exit(1);
   }
   abandon_children(); // (two seconds for the orderly exit, then SIGKILL: a rank may be inside a collective)
   alarm(0);
   std::cerr << cli::timestamp() << "Exception: " << mg.sh->msg << std::endl << cli::timestamp() << "Terminating" << std::endl;
   if (ctx) fpca_destroy(ctx);
   return EXIT_FAILURE;
}

void multi_on_exception()
{
   if (g_child_rank > 0) {
      if (g_shared) g_shared->failed.fetch_add(1);
      _exit(1);
   }
   abandon_children(); // rank 0 of a --gpus run: the others must not wait for it
}

bool multi_connect(Multi &mg, fpca_ctx **ctx, const char *bed_file, uint64_t N, int stand_method, int device, int accum, uint64_t *nsnps)
{
   if (mg.sh->failed.load() == 0) {
      if (fpca_create_from_bed(ctx, bed_file, N, mg.snp_begin, mg.snp_count, stand_method, device, accum, nsnps) != FPCA_OK)
         multi_fail(mg, fpca_last_error());
      else if (fpca_set_total_snps(*ctx, *nsnps) != FPCA_OK)
         multi_fail(mg, fpca_last_error());
   }
   if (!multi_barrier(mg)) return false;
#ifdef FPCA_TEST_HOOKS
   if (mg.test_transport) {
      // failure injection for tests/test_cli.py (test transport only): rank R kills itself / rank 0 throws after the
      // fork -- the run must end with a message and a non-zero status instead of hanging
      if (const char *kr = FPCA_TEST_ENV("FPCA_CLI_TEST_KILL_RANK")) {
         if (atoi(kr) == mg.rank && mg.rank > 0) raise(SIGKILL);
         if (atoi(kr) == 0 && mg.rank == 0) throw std::runtime_error("injected failure of rank 0 after the fork");
      }
      if (fpca_set_allreduce(*ctx, shm_allreduce, &mg) != FPCA_OK || fpca_set_rank(*ctx, mg.ngpus, mg.rank) != FPCA_OK)
         multi_fail(mg, fpca_last_error());
      if (mg.test_collectives && fpca_set_collectives(*ctx, shm_allgather, shm_reducescatter, &mg) != FPCA_OK) multi_fail(mg, fpca_last_error());
   } else
#endif
   {
      if (mg.rank == 0) {
         if (fpca_comm_unique_id(mg.sh->id) != FPCA_OK) multi_fail(mg, fpca_last_error());
         mg.sh->id_ready.store(1);
      } else
         while (!mg.sh->id_ready.load() && !mg.sh->failed.load()) sched_yield();
      if (mg.sh->failed.load() == 0 && fpca_comm_init_rank(*ctx, mg.ngpus, mg.rank, mg.sh->id) != FPCA_OK) multi_fail(mg, fpca_last_error());
   }
   return multi_barrier(mg);
}

// Eigenvectors / PCs need no gather: every rank has downloaded ITS OWN ROWS straight into the shared region (m.U, m.Px).  Loadings
// and mean/sd are this shard's rows and go into the region at their place.
bool multi_collect(Multi &mg, fpca_ctx *ctx, int n_dim, uint64_t nsnps, const double *Vloc, const double *msloc, double *V, double *meansd)
{
   const uint64_t P_loc = fpca_nsnps(ctx);
   for (int c = 0; c < n_dim && Vloc; c++) std::memcpy(mg.V + (size_t)c * nsnps + mg.snp_begin, Vloc + (size_t)c * P_loc, P_loc * sizeof(double));
   for (int c = 0; c < 2; c++) std::memcpy(mg.meansd + (size_t)c * nsnps + mg.snp_begin, msloc + (size_t)c * P_loc, P_loc * sizeof(double));
   const bool all_ok = multi_barrier(mg);
   if (mg.rank > 0) {
      fpca_destroy(ctx);
      _exit(all_ok ? 0 : 1); // (rank 0 reports "not converged": every rank got the same rc)
   }
   if (!all_ok) return false;
   wait_children();
   if (Vloc) std::memcpy(V, mg.V, (size_t)nsnps * n_dim * sizeof(double));
   std::memcpy(meansd, mg.meansd, (size_t)nsnps * 2 * sizeof(double));
   return true;
}
