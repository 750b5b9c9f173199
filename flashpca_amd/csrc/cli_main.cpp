// cli_main.cpp -- `flashpca`, drop-in for the reference CLI's PCA modes (flashpca.cpp:30-895) on MI355X: the run itself.
//
// Same flags and defaults as the reference (cli_options.cpp), same stdout milestones and the same output files / format
// (eigenvalues / eigenvectors / pcs / pve [/ loadings / meansd], flashpca.cpp:755-878).  Host C++ only: all arithmetic goes
// through the C ABI of libfpca.so (include/fpca.h); there is no CPU compute path.  Besides PCA, --check and --project, --ucca
// (per-SNP association with the --pheno phenotypes, RandomPCA::ucca) runs on one GPU; --scca is refused (the library has sparse
// CCA, fpca_scca_prepare / fpca_scca_fit; the flag and its output files are not wired to it).
// main() is a sequence of steps over one `Run`: options (cli_options.cpp) -> .fam / .bim / subset lists / phenotypes -> what the
// file sizes refuse -> with --gpus, the launcher (cli_multi.cpp) -> device context -> run_pca | run_check | run_ucca |
// run_project -> write_outputs -> _exit.
#include <algorithm>
#include <cerrno>
#include <chrono>
#include <cmath>
#include <csignal>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <future>
#include <iostream>
#include <memory>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include <execinfo.h>
#include <sys/stat.h>
#include <unistd.h>

#include "cli_multi.hpp"
#include "cli_options.hpp"
#include "common.hpp"
#include "plink_io.hpp"

using namespace cli;

namespace {

void fpca_ok(int rc)
{
   if (rc != FPCA_OK) throw std::runtime_error(fpca_last_error());
}

// the big results live in UNINITIALISED memory: a std::vector would zero 80 + 80 + 16 MB on this thread first (35 ms of
// page faults at 500,000 x 100,000); the parallel download touches the pages instead
struct Buf {
   std::unique_ptr<double[]> p;
   size_t n = 0;
   void resize(size_t k)
   {
      p.reset(new double[k]);
      n = k;
   }
   double *data() { return p.get(); }
   bool empty() const { return n == 0; }
};

struct Joiner { // joins its threads on every way out of its scope, exceptions included
   std::vector<std::thread> th;
   ~Joiner()
   {
      for (auto &t : th)
         if (t.joinable()) t.join();
   }
};

// FPCA_TIMING=1: wall-clock of each phase on stderr
struct PhaseTimer {
   bool on = std::getenv("FPCA_TIMING") != nullptr; // (main() turns it off in ranks > 0 of a --gpus run)
   std::chrono::steady_clock::time_point last = std::chrono::steady_clock::now();
   void operator()(const char *what)
   {
      const auto now = std::chrono::steady_clock::now();
      if (on) std::fprintf(stderr, "[fpca-cli] %-32s %8.3f ms\n", what, std::chrono::duration<double>(now - last).count() * 1e3);
      last = now;
   }
};

// what the steps of one run share
struct Run {
   const Options &o;
   PhaseTimer phase;
   std::vector<std::string> snp_ids, ref_alleles, alt_alleles, fam_ids, indiv_ids;
   uint64_t N = 0;      // samples of the fileset
   uint64_t N_pca = 0;  // samples of the eigenproblem (--keep / --remove)
   uint64_t P_file = 0; // SNPs in the .bed, from the file size alone (data.cpp:165-170) -- known before any device work
   uint64_t nsnps = 0;  // the same, as the library found it (all shards)
   std::vector<uint8_t> keep_mask;
   std::vector<uint64_t> kept_rows;
   fpca::TextMatrix pheno;
   Multi mg;
   fpca_ctx *ctx = nullptr;
   Buf U, Px, V;
   std::vector<double> d, pve, meansd, ucca_res;
   int k_out = 0;
   std::vector<std::string> rownames, rn_snp; // "FID\tIID" / "SNP\tRefAllele" row labels of the output files
   Joiner helpers;                            // (last: joined before anything the threads write is destroyed)
   explicit Run(const Options &opts) : o(opts), k_out(opts.n_dim) { helpers.th.reserve(8); }
};

void sample_labels(Run &r, uint64_t begin, uint64_t end)
{
   for (uint64_t i = begin; i < end; i++) r.rownames[i] = r.fam_ids[i] + "\t" + r.indiv_ids[i];
}
void snp_labels(Run &r)
{
   r.rn_snp.resize(r.snp_ids.size());
   for (size_t i = 0; i < r.rn_snp.size(); i++) r.rn_snp[i] = r.snp_ids[i] + "\t" + r.ref_alleles[i];
}
// {first, stem1, ..., stemk}: the header line of an output file
std::vector<std::string> numbered(const char *first, const char *stem, int k)
{
   std::vector<std::string> names{first};
   for (int i = 1; i <= k; i++) names.push_back(stem + std::to_string(i));
   return names;
}

// One GPU: the HIP runtime starts up (~0.1 s) on a helper thread while this one reads the text files, and the .bim is
// parsed on another while the .fam is (only N, from the .fam, is needed before the upload can start).  With --gpus the
// parent must not touch HIP, nor hold threads, before it forks: everything stays on this thread.
void read_text_files(Run &r)
{
   const Options &o = r.o;
   if (o.ngpus == 1) r.helpers.th.emplace_back([device = o.device] { (void)fpca_warmup(device); }); // (errors resurface in fpca_create_from_bed)
   auto parse_bim = [&] { fpca::read_plink_bim(o.bim_file, r.snp_ids, r.ref_alleles, r.alt_alleles); };
   std::future<void> bim; // (a thread of its own; joined by get(), or by the destructor if read_fam throws)
   if (o.ngpus == 1) bim = std::async(std::launch::async, parse_bim);
   // N = number of rows of the .fam whose 6th column parses as a number (flashpca.cpp:589 -> data.cpp:408-413), and the
   // two id columns (read_plink_fam, flashpca.cpp:591) from the same pass over the file
   r.N = fpca::read_fam(o.fam_file, r.fam_ids, r.indiv_ids);
   if (bim.valid()) bim.get(); // (rethrows what the .bim parse threw)
   else parse_bim();
   if (r.N == 0) throw std::runtime_error("no samples found in " + o.fam_file);
   // --keep / --remove: the samples the PCA runs on (everything about the lists is checked here, before any device work)
   if (o.subset) {
      r.keep_mask = fpca::read_sample_subset(r.fam_ids, r.indiv_ids, o.keep_file, o.remove_file);
      for (uint64_t i = 0; i < r.N; i++)
         if (r.keep_mask[i]) r.kept_rows.push_back(i);
      if (r.kept_rows.size() < 2)
         throw UsageError("--keep / --remove leave " + std::to_string(r.kept_rows.size()) + " of " + std::to_string(r.N) + " samples, at least 2 are needed");
      o.verbose && std::cout << timestamp() << "PCA on " << r.kept_rows.size() << " of " << r.N << " samples (--keep / --remove)" << std::endl;
   }
   r.N_pca = o.subset ? r.kept_rows.size() : r.N;
   r.phase(".fam / .bim");
   // UCCA: the phenotypes (Data::read_pheno(pheno, 3), data.cpp:408-413), checked against the .fam before any device work.  The
   // reference takes N from this file's rows and then reads the .bed with that N whatever the .fam says; this build refuses.
   if (o.mode == MODE_UCCA) {
      r.pheno = fpca::read_text(o.pheno_file, 3);
      if (r.pheno.rows != r.N)
         throw UsageError("the phenotype file " + o.pheno_file + " has " + std::to_string(r.pheno.rows) + " rows, but " + o.fam_file + " has " +
                          std::to_string(r.N) + " samples");
      if (r.pheno.cols < 1 || r.pheno.cols + 2 > r.N)
         throw UsageError("UCCA needs between 1 and N - 2 = " + std::to_string(r.N >= 2 ? r.N - 2 : 0) + " phenotypes, the phenotype file has " +
                          std::to_string(r.pheno.cols));
      r.phase("phenotypes");
   }
}

// everything that can be refused from the file sizes alone is refused here: before any device work, and -- in a
// --gpus run -- before the fork, so that no rank is left waiting for another
void check_file_sizes(Run &r)
{
   const Options &o = r.o;
   struct stat st;
   if (stat(o.geno_file.c_str(), &st) != 0) throw std::runtime_error("[Data::read_bed] Error reading file " + o.geno_file + ", error " + strerror(errno));
   r.P_file = (uint64_t)st.st_size > 3 ? ((uint64_t)st.st_size - 3) / ((r.N + 3) / 4) : 0; // data.cpp:165-170
   // flashpca.cpp:623-633
   const unsigned max_dim = (unsigned)((std::fmin((double)r.N_pca, (double)r.P_file) - 1) / 2.0);
   if ((unsigned)o.n_dim > max_dim) // (every mode, like the reference)
      throw UsageError("You asked for " + std::to_string(o.n_dim) + " dimensions, but only " + std::to_string(max_dim) + "allowed");
   // the loadings / mean-sd files carry one .bim row name per SNP of the .bed
   if ((o.do_loadings || o.save_meansd) && r.snp_ids.size() != r.P_file)
      throw std::runtime_error("the .bim file has a different number of SNPs (" + std::to_string(r.snp_ids.size()) + ") than the .bed (" +
                               std::to_string(r.P_file) + ")");
}

// Opens the .bed on the device (one GPU), or this rank's shard of it and the transport (--gpus; false: a rank failed).
bool create_context(Run &r)
{
   const Options &o = r.o;
   const int my_device = o.device + ((o.ngpus > 1 && !r.mg.test_transport) ? r.mg.rank : 0);
   if (o.ngpus == 1) {
      // One GPU, PCA: while the .bed streams to the device (that is the copy engine's and the reader threads' business), a
      // helper thread gets the host side of the results ready -- it touches the pages of the 80 + 80 + 16 MB result buffers
      // (first-touch page faults are 35 ms of a one-threaded pass, and the download would otherwise pay them) and builds the
      // row labels of the output files.
      std::thread *prep = nullptr;
      if (o.mode == MODE_PCA && r.P_file > 0) {
         r.U.resize((size_t)r.N * o.n_dim);
         r.Px.resize((size_t)r.N * o.n_dim);
         if (o.do_loadings) r.V.resize((size_t)r.P_file * o.n_dim);
         r.helpers.th.emplace_back([&r] {
            for (Buf *bf : {&r.U, &r.Px, &r.V})
               for (size_t i = 0; i < bf->n; i += 512) bf->p[i] = 0.0; // one write per 4 KB page
            r.rownames.resize(r.N);
            sample_labels(r, 0, r.N);
            if ((r.o.do_loadings || r.o.save_meansd) && r.snp_ids.size() == r.P_file) snp_labels(r);
         });
         prep = &r.helpers.th.back();
      }
      fpca_ok(fpca_create_from_bed(&r.ctx, o.geno_file.c_str(), r.N, 0, 0, o.stand_method_x, o.device, o.accum, &r.nsnps));
      if (prep) prep->join();
   } else if (!multi_connect(r.mg, &r.ctx, o.geno_file.c_str(), r.N, o.stand_method_x, my_device, o.accum, &r.nsnps))
      return false;
   r.phase("device init + .bed upload");
   o.verbose && std::cout << timestamp() << "Detected BED file: " << o.geno_file << " with " << r.N << " samples, " << r.nsnps << " SNPs." << std::endl;
   if (o.verbose) {
      char name[256];
      if (fpca_device_name(my_device, name, sizeof(name)) == FPCA_OK) std::cout << timestamp() << "Device " << my_device << ": " << name << std::endl;
      if (o.ngpus > 1)
         std::cout << timestamp() << o.ngpus << " GPUs, " << r.mg.snp_count << " SNPs on this one; transport: "
                   << (r.mg.test_transport ? "host shared memory (test)" : "RCCL") << std::endl;
   }
   // the reference prints its dense block geometry here (flashpca.cpp:688-690); the whole packed matrix is one resident block
   std::cout << timestamp() << "blocksize: " << r.nsnps << " (" << (long long)((r.N + 3) / 4) * (long long)r.nsnps << " bytes per block)" << std::endl;
   return true;
}

// false: a rank of the --gpus run failed
bool run_pca(Run &r)
{
   const Options &o = r.o;
   const int n_dim = o.n_dim;
   const uint64_t N = r.N, nsnps = r.nsnps;
   std::cout << timestamp() << "PCA begin" << std::endl;
   fpca_pca_opts po;
   FPCA_PCA_OPTS_INIT(&po);
   po.ndim = n_dim;
   po.blockvec = o.blockvec;
   po.maxiter = o.maxiter;
   po.tol = o.tol;
   po.divisor = o.divisor;
   po.do_loadings = o.do_loadings ? 1 : 0;
   po.max_blocks = o.maxblocks;
   po.mixed = o.mixed;
   po.replicated_solver = o.replicated_solver;
   po.verbose = o.verbose ? 1 : 0;
   po.seed = (uint64_t)o.seed;
   r.d.resize(n_dim);
   r.pve.resize(n_dim);
   r.meansd.resize((size_t)nsnps * 2);
   fpca_pca_info info;
   int rc;
   if (o.ngpus == 1) {
      if (r.U.empty()) r.U.resize((size_t)N * n_dim);
      if (r.Px.empty()) r.Px.resize((size_t)N * n_dim);
      if (o.do_loadings && (r.V.empty() || nsnps != r.P_file)) r.V.resize((size_t)nsnps * n_dim);
      if (o.subset) fpca_ok(fpca_set_sample_mask(r.ctx, r.keep_mask.data()));
      rc = fpca_pca(r.ctx, &po, r.U.data(), r.d.data(), r.Px.data(), r.pve.data(), o.do_loadings ? r.V.data() : nullptr, r.meansd.data(), &info);
   } else {
      // Eigenvectors / PCs: every rank downloads ITS OWN ROWS (its slice of the row-sharded basis, or an even share of the
      // replicated one) straight into the shared region -- no gather of the Ritz blocks, no funnel through rank 0's PCIe
      // link; loadings and mean/sd are this shard's rows, gathered by multi_collect
      const uint64_t P_loc = fpca_nsnps(r.ctx);
      std::vector<double> Vloc, msloc((size_t)P_loc * 2);
      if (o.do_loadings) Vloc.resize((size_t)P_loc * n_dim);
      if (r.mg.rank > 0) po.verbose = 0;
      po.partial_rows = 1;
      rc = fpca_pca(r.ctx, &po, r.mg.U, r.d.data(), r.mg.Px, r.pve.data(), o.do_loadings ? Vloc.data() : nullptr, msloc.data(), &info);
      if (rc != FPCA_OK && rc != FPCA_ENOTCONVERGED) multi_fail(r.mg, fpca_last_error());
      if (o.do_loadings && r.mg.rank == 0) r.V.resize((size_t)nsnps * n_dim); // (rank 0 alone has all the rows, after the gather)
      if (!multi_collect(r.mg, r.ctx, n_dim, nsnps, o.do_loadings ? Vloc.data() : nullptr, msloc.data(), r.V.data(), r.meansd.data())) return false;
   }
   if (rc == FPCA_ENOTCONVERGED) // randompca.cpp:210-217
      throw std::runtime_error("Spectra eigen-decomposition was not successful, status: not converging");
   fpca_ok(rc);
   o.verbose && std::cout << timestamp() << "GRM trace: " << info.trace << std::endl;
   o.verbose && std::cout << timestamp() << info.block_applies << " block applies of width " << info.blockvec << " (" << info.vector_ops
                          << " vector operations), " << info.restarts << " restarts, device " << info.seconds_apply + info.seconds_ortho
                          << " s, host " << info.seconds_host << " s" << std::endl;
   if (o.verbose && info.cheap_applies > 0)
      std::cout << timestamp() << info.cheap_applies << " of the block applies on " << info.cheap_slices
                << " byte slices of the operand, verified by exact passes" << std::endl;
   if (o.verbose && o.ngpus > 1) {
      static const char *const names[] = {"single", "row-sharded", "replicated", "replicated (the self-test of the row-sharded exchange failed)",
                                          "replicated (a collective of the row-sharded solve failed; started over)"};
      std::cout << timestamp() << "eigensolver layout over " << o.ngpus << " GPUs: " << names[info.solver_path >= 0 && info.solver_path <= 4 ? info.solver_path : 0]
                << std::endl;
      uint64_t ccalls = 0, cbytes = 0;
      if (fpca_collective_stats(r.ctx, &ccalls, &cbytes) == FPCA_OK)
         std::cout << timestamp() << "collectives on the data path: " << ccalls << " calls, " << cbytes << " bytes sent per rank" << std::endl;
   }
   std::cout << timestamp() << "PCA done" << std::endl;
   return true;
}

// RandomPCA::check(Data&, block_size, evec_file, eval_file) (randompca.cpp:627-661)
void run_check(Run &r)
{
   const bool verbose = r.o.verbose;
   fpca::TextMatrix ev = fpca::read_text(r.o.eigvalfile, 1, -1, 0);
   if (ev.rows == 0) throw std::runtime_error("No eigenvalues found in file");
   fpca::TextMatrix evec = fpca::read_text(r.o.eigvecfile, 3, -1, 1);
   if (evec.rows != r.N)
      throw std::runtime_error("Eigenvector dimension doesn't match data dimension (evec.rows = " + std::to_string(evec.rows) +
                               "; dat.N = " + std::to_string(r.N) + ")");
   if (ev.rows != evec.cols) throw std::runtime_error("Eigenvector dimension doesn't match the number of eigenvalues");
   const int K = (int)evec.cols;
   std::vector<double> err(K);
   double mse = 0, rmse = 0;
   fpca_ok(fpca_check(r.ctx, evec.v.data(), (int64_t)r.N, ev.v.data(), K, r.o.divisor, err.data(), &mse, &rmse));
   // printed under --verbose only, like the reference (randompca.cpp:670-700)
   verbose && std::cout << timestamp() << "Checking mean square error between (X X' U) / div and (U D^2) for " << K << " dimensions" << std::endl;
   for (int j = 0; j < K; j++)
      verbose && std::cout << timestamp() << "eval(" << (j + 1) << "): " << ev.v[j] << ", sum squared error: " << err[j] << std::endl;
   verbose && std::cout << timestamp() << "Mean squared error: " << mse << ", Root mean squared error: " << rmse << " (n=" << r.N << ")" << std::endl;
}

// flashpca.cpp:729-737 -> RandomPCA::ucca(Data&) (randompca.cpp:567-625)
void run_ucca(Run &r)
{
   std::cout << timestamp() << "UCCA begin" << std::endl;
   r.o.verbose && std::cout << timestamp() << "UCCA online mode, N=" << r.N << " p=" << r.nsnps << std::endl;
   r.ucca_res.resize((size_t)r.nsnps * 3);
   fpca_ok(fpca_ucca(r.ctx, r.pheno.v.data(), (int64_t)r.N, (int)r.pheno.cols, r.o.stand_method_y, r.ucca_res.data(), (int64_t)r.nsnps));
   std::cout << timestamp() << "UCCA done" << std::endl;
}

// RandomPCA::project (randompca.cpp:745-820)
void run_project(Run &r)
{
   const Options &o = r.o;
   const uint64_t nsnps = r.nsnps;
   fpca::TextMatrix L = fpca::read_text(o.in_load_file, 3, -1, 1);
   if (L.rows != nsnps) throw std::runtime_error("number of SNPs in the loadings file doesn't match the data");
   std::vector<double> ms((size_t)nsnps * 2);
   if (!o.in_maf_file.empty()) {
      std::vector<double> maf = fpca::read_maf(o.in_maf_file, r.snp_ids);
      if (maf.size() != nsnps) throw std::runtime_error("number of SNPs in the MAF file doesn't match the data");
      for (uint64_t j = 0; j < nsnps; j++) { // maf2meansd (randompca.cpp:737-743), including its missing sqrt
         ms[j] = maf[j] * 2.0;
         ms[nsnps + j] = maf[j] * 2.0 * (1.0 - maf[j]);
      }
   } else {
      fpca::TextMatrix M2 = fpca::read_text(o.in_meansd_file, 3, -1, 1);
      if (M2.rows != nsnps || M2.cols < 2) throw std::runtime_error("mean/sd file doesn't match the data");
      for (uint64_t j = 0; j < nsnps; j++) {
         ms[j] = M2.at(j, 0);
         ms[nsnps + j] = M2.at(j, 1);
      }
   }
   fpca_ok(fpca_set_meansd(r.ctx, ms.data()));
   r.k_out = (int)L.cols;
   r.Px.resize((size_t)r.N * r.k_out);
   fpca_ok(fpca_apply_x(r.ctx, L.v.data(), (int64_t)nsnps, r.k_out, r.Px.data(), (int64_t)r.N));
   double div = 1;
   if (o.divisor == FPCA_DIVISOR_N1) div = (double)r.N - 1;
   else if (o.divisor == FPCA_DIVISOR_P) div = (double)L.rows;
   const double s = std::sqrt(div);
   for (size_t i = 0; i < r.Px.n; i++) r.Px.p[i] /= s; // randompca.cpp:818
}

// ---- write out results (flashpca.cpp:755-878) --------------------------------------------------------
// The files -- eigenvectors, PCs and loadings are 140 + 140 + 28 MB of text at 500,000 x 100,000 -- are written one
// after the other, each by an in-order writer fed by every CPU this process may use (plink_io.cpp save_text: formatting
// 22 million numbers IS the output phase; three files at once on a third of the CPUs each measured no faster), while
// the device context (25 GB to give back) is torn down on another thread.
void write_outputs(Run &r)
{
   const Options &o = r.o;
   const uint64_t nsnps = r.nsnps;
   const int precision = o.precision;
   const unsigned cpus = fpca::usable_cpus();
   if (r.phase.on) std::fprintf(stderr, "[fpca-cli] usable CPUs: %u\n", cpus);
   auto sample_rownames = [&] {
      if (r.rownames.size() == r.N) return; // (built beside the upload)
      r.rownames.resize(r.N);
      const unsigned nt = std::max(1u, std::min(cpus, 8u));
      Joiner part;
      for (unsigned t = 0; t < nt; t++) part.th.emplace_back([&r, t, nt] { sample_labels(r, r.N * t / nt, r.N * (t + 1) / nt); });
   };
   auto snp_rownames = [&] {
      if (!r.rn_snp.empty()) return;
      snp_labels(r);
      if (r.rn_snp.size() != nsnps) throw std::runtime_error("the .bim file has a different number of SNPs than the .bed");
   };
   if (o.save_meansd && r.meansd.empty()) { // (--project / --check: the statistics are still on the device)
      r.meansd.resize((size_t)nsnps * 2);
      fpca_ok(fpca_stats(r.ctx, r.meansd.data(), nullptr));
   }
   Joiner teardown; // (joined on every way out: it refers to this run)
   teardown.th.emplace_back([&r] { fpca_destroy(r.ctx); }); // nothing below needs the device
   if (o.mode == MODE_PCA) {
      const int n_dim = o.n_dim;
      const std::vector<std::string> none;
      std::cout << timestamp() << "Writing " << n_dim << " eigenvalues to file " << o.eigvalfile << std::endl;
      fpca::save_text(r.d.data(), n_dim, 1, none, none, o.eigvalfile, precision);

      sample_rownames();
      const std::vector<std::string> colnames_u = numbered("FID\tIID", "U", n_dim), colnames_pc = numbered("FID\tIID", "PC", n_dim);
      const double *U_all = o.ngpus > 1 ? r.mg.U : r.U.data(), *Px_all = o.ngpus > 1 ? r.mg.Px : r.Px.data(); // (--gpus: the shared region)
      // --keep / --remove: the samples of the PCA only, in .fam order: what a run on the subset fileset writes
      std::vector<std::string> rn_kept(o.subset ? r.N_pca : 0);
      std::vector<double> Mk(o.subset ? (size_t)r.N_pca * n_dim : 0);
      for (size_t i = 0; i < rn_kept.size(); i++) rn_kept[i] = r.rownames[r.kept_rows[i]];
      auto save_pca_rows = [&](const double *M, const std::vector<std::string> &colnames, const std::string &file) {
         for (int j = 0; j < n_dim && o.subset; j++)
            for (uint64_t i = 0; i < r.N_pca; i++) Mk[i + (size_t)j * r.N_pca] = M[r.kept_rows[i] + (size_t)j * r.N];
         fpca::save_text(o.subset ? Mk.data() : M, r.N_pca, n_dim, colnames, o.subset ? rn_kept : r.rownames, file, precision, cpus);
      };
      std::cout << timestamp() << "Writing " << n_dim << " eigenvectors to file " << o.eigvecfile << std::endl;
      save_pca_rows(U_all, colnames_u, o.eigvecfile);
      std::cout << timestamp() << "Writing " << n_dim << " PCs to file " << o.pcfile << std::endl;
      save_pca_rows(Px_all, colnames_pc, o.pcfile);
      if (!o.pcallfile.empty()) {
         std::cout << timestamp() << "Writing " << n_dim << " PCs of all " << r.N << " samples to file " << o.pcallfile << std::endl;
         fpca::save_text(Px_all, r.N, n_dim, colnames_pc, r.rownames, o.pcallfile, precision, cpus);
      }

      std::cout << timestamp() << "Writing " << n_dim << " proportion variance explained to file " << o.eigpvefile << std::endl;
      fpca::save_text(r.pve.data(), n_dim, 1, none, none, o.eigpvefile, precision);

      if (o.do_loadings) {
         std::cout << timestamp() << "Writing SNP loadings to file " << o.loadingsfile << std::endl;
         snp_rownames();
         fpca::save_text(r.V.data(), nsnps, n_dim, numbered("SNP\tRefAllele", "V", n_dim), r.rn_snp, o.loadingsfile, precision, cpus);
      }
   } else if (o.mode == MODE_PROJECT) {
      sample_rownames();
      fpca::save_text(r.Px.data(), r.N, r.k_out, numbered("FID\tIID", "PC", r.k_out), r.rownames, o.projfile, precision);
   } else if (o.mode == MODE_UCCA) { // flashpca.cpp:846-852: one row per .bim SNP, named by its id
      if (r.snp_ids.size() != nsnps) throw std::runtime_error("the .bim file has a different number of SNPs than the .bed");
      fpca::save_text(r.ucca_res.data(), nsnps, 3, {"SNP", "R", "Fstat", "P"}, r.snp_ids, o.uccafile, precision);
   }
   if (o.save_meansd) {
      std::cout << timestamp() << "Writing mean + sd file " << o.meansdfile << std::endl;
      snp_rownames();
      fpca::save_text(r.meansd.data(), nsnps, 2, {"SNP\tRefAllele", "Mean", "SD"}, r.rn_snp, o.meansdfile, precision);
   }
}

} // namespace

#ifdef FPCA_TEST_HOOKS
static void on_segv(int)
{
   void *bt[64];
   const int n = backtrace(bt, 64);
   backtrace_symbols_fd(bt, n, 2);
   _exit(139);
}
#endif

int main(int argc, char *argv[])
{
#ifdef FPCA_TEST_HOOKS
   signal(SIGSEGV, on_segv);
#endif
   VarMap vm;
   try {
      vm = parse_command_line(argc, argv);
   } catch (std::exception &e) {
      // flashpca.cpp:100-106 (exit status is EXIT_SUCCESS there too)
      std::cerr << e.what() << std::endl << "Use --help to get more help" << std::endl;
      return EXIT_SUCCESS;
   }
   show_timestamp = !vm.count("notime");

   std::cout << timestamp() << "arguments: flashpca ";
   for (int i = 0; i < argc; i++) std::cout << argv[i] << " ";
   std::cout << std::endl;

   if (vm.count("version") || vm.count("help")) {
      std::cerr << "flashpca " << FLASHPCA_VERSION << std::endl;
      if (vm.count("version"))
         std::cerr << "MI355X-native implementation of the flashpca 2.1 PCA path (command line after Gad Abraham's flashpca)." << std::endl << std::endl;
      else
         print_help();
      return EXIT_SUCCESS;
   }

   try {
      const Options o = validate(vm);
      std::cout << timestamp() << "Start flashpca (version " << FLASHPCA_VERSION << ")" << std::endl;
      o.verbose && std::cout << timestamp() << "seed: " << o.seed << std::endl;

      Run r(o);
      read_text_files(r);
      check_file_sizes(r);
      if (o.ngpus > 1) {
         multi_launch(r.mg, o.ngpus, r.N, r.P_file, o.n_dim);
         r.phase.on &= r.mg.rank == 0;
      }
      if (!create_context(r)) return multi_abort(r.mg, r.ctx);
      if (o.mode == MODE_PCA && !run_pca(r)) return multi_abort(r.mg, r.ctx);
      if (o.mode == MODE_CHECK) run_check(r);
      if (o.mode == MODE_UCCA) run_ucca(r);
      if (o.mode == MODE_PROJECT) run_project(r);
      r.phase("compute");
      write_outputs(r);
      r.phase("output files + teardown");
      std::cout << timestamp() << "Goodbye!" << std::endl;
      // every file is closed and the context destroyed: leave without running the HIP runtime's static destructors
      // (tens of milliseconds of unloading code objects and tearing down queues that nobody waits for)
      std::cout.flush();
      std::fflush(nullptr);
      _exit(EXIT_SUCCESS);
   } catch (UsageError &e) { // (always before any device work and before the fork)
      std::cerr << "Error: " << e.what() << std::endl;
      if (e.with_help_hint) std::cerr << "Use --help to get more help" << std::endl;
      return EXIT_FAILURE;
   } catch (std::exception &e) {
      std::cerr << timestamp() << "Exception: " << e.what() << std::endl;
      std::cerr << timestamp() << "Terminating" << std::endl;
   } catch (...) {
      std::cerr << timestamp() << "Caught unknown exception, terminating " << std::endl;
   }
   multi_on_exception(); // a child of a --gpus run exits here; rank 0 winds the others down
   return EXIT_FAILURE;
}
