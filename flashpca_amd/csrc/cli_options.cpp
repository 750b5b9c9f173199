// cli_options.cpp -- the options of `flashpca`: the reference's flags (flashpca.cpp:41-92) with its defaults (ndim 10, standx
// binom2, div p, tol 1e-6, maxiter 500, precision 7, suffix .txt), parsed like boost::program_options parses them, and this
// build's own (--device, --gpus, --solver, --blockvec, --maxblocks, --passes, --keep, --remove, --outpcall, --accum).
// --memory / --blocksize / --batch / --numthreads are checked and otherwise ignored: the packed matrix is always resident in HBM.
#include "cli_options.hpp"

#include <cerrno>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <initializer_list>
#include <iostream>
#include <vector>

namespace cli {

bool show_timestamp = true;

std::string timestamp()
{
   if (!show_timestamp) return "";
   time_t t = time(nullptr);
   char *s = asctime(localtime(&t));
   s[strlen(s) - 1] = '\0';
   return std::string("[") + s + "] ";
}

namespace {

struct OptSpec {
   const char *name;
   char shortname;
   bool has_value;
   const char *help;
   bool ext = false; // an option this build adds: matched by its full name only, so that every abbreviation the reference
                     // accepts (boost::program_options guesses unambiguous prefixes, flashpca.cpp:97) still means what it meant
};

const OptSpec OPTS[] = {
   {"help", 0, false, "produce help message"},
   {"scca", 0, false, "perform sparse canonical correlation analysis (SCCA) [not supported by this build]"},
   {"ucca", 0, false, "perform per-SNP canonical correlation analysis (UCCA): one F test of all --pheno phenotypes per SNP, written to ucca<suffix>"},
   {"project", 'p', false, "project new samples onto existing principal components"},
   {"batch", 0, false, "load all genotypes into RAM at once (no effect: the packed matrix is always resident in HBM)"},
   {"memory", 'm', true, "size of block, in MB (no effect)"},
   {"blocksize", 'b', true, "size of block for, in number of SNPs (no effect)"},
   {"numthreads", 'n', true, "set number of OpenMP threads (no effect)"},
   {"seed", 0, true, "set random seed"},
   {"bed", 0, true, "PLINK bed file"},
   {"bim", 0, true, "PLINK bim file"},
   {"fam", 0, true, "PLINK fam file"},
   {"pheno", 0, true, "PLINK phenotype file (UCCA: FID, IID, then one column per phenotype; one row per .fam sample)"},
   {"bfile", 0, true, "PLINK root name"},
   {"ndim", 'd', true, "number of PCs to output"},
   {"standx", 's', true, "standardization method for genotypes [binom2 | binom]"},
   {"standy", 0, true, "standardization method for phenotypes in UCCA mode [sd | binom2 | binom | none | center] (default sd; ignored by PCA)"},
   {"div", 0, true, "whether to divide the eigenvalues by p, n - 1, or don't divide [p | n1 | none]"},
   {"outpc", 0, true, "PC output file"},
   {"outpcx", 0, true, "X PC output file, for CCA (ignored)"},
   {"outpcy", 0, true, "Y PC output file, for CCA (ignored)"},
   {"outvec", 0, true, "eigenvector output file"},
   {"outload", 0, true, "SNP loadings"},
   {"outvecx", 0, true, "X eigenvector output file, for CCA (ignored)"},
   {"outvecy", 0, true, "Y eigenvector output file, for CCA (ignored)"},
   {"outval", 0, true, "Eigenvalue output file"},
   {"outpve", 0, true, "proportion of variance explained output file"},
   {"outmeansd", 0, true, "mean+SD (used to standardize SNPs) output file"},
   {"outproj", 0, true, "PCA projection output file"},
   {"inload", 0, true, "SNP loadings input file"},
   {"inmeansd", 0, true, "mean+SD (used to standardize SNPs) input file"},
   {"inmaf", 0, true, "MAF input file"},
   {"verbose", 'v', false, "verbose"},
   {"tol", 0, true, "tolerance for PCA iterations"},
   {"lambda1", 0, true, "1st penalty for CCA/SCCA (ignored)"},
   {"lambda2", 0, true, "2nd penalty for CCA/SCCA (ignored)"},
   {"maxiter", 0, true, "maximum number of iterations: restarts of the reference's 2 ndim + 1 vector Lanczos factorisation, i.e. a budget of 2 ndim + 1 + maxiter (ndim + 1) operator applications"},
   {"debug", 0, false, "debug (no effect)"},
   {"suffix", 'f', true, "suffix for all output files"},
   {"check", 'c', false, "check eigenvalues/eigenvectors"},
   {"precision", 0, true, "digits of precision for output"},
   {"notime", 0, false, "don't print timestamp in output"},
   {"save-vinit", 0, false, "saves the initial v eigenvector for SCCA (no effect)"},
   {"version", 0, false, "version"},
   {"device", 0, true, "HIP device index [0] (with --gpus G: the first of G consecutive devices)", true},
   {"gpus", 0, true, "number of GPUs for PCA [1]: the SNPs are split into that many contiguous shards, one process per GPU, partial products summed over RCCL", true},
   {"solver", 0, true, "with --gpus: how the eigensolver's sample-sized work is laid out [rowshard | replicated]: rowshard (default) = every GPU keeps and orthogonalises 1/G of the rows of the Krylov basis (all-gather -> products -> reduce-scatter per pass); replicated = every GPU keeps the whole basis, ONE all-reduce of the N x b product per pass and nothing else on the wire.  rowshard checks its exchange once and falls back to replicated by itself if the check fails", true},
   {"blockvec", 0, true, "block width of the eigensolver: 16, 32, 48 or 64 [16; 32 / 64 for ndim > 64 / > 128]", true},
   {"maxblocks", 0, true, "basis cap (in blocks) before a thick restart [automatic]", true},
   {"passes", 0, true, "arithmetic of the eigensolver's passes in the exact-integer modes [mixed | exact]: mixed (default) = a solve that needs many passes makes most of them on 4 byte slices of the fp64 operand and puts the Ritz vectors through the exact operator before it declares convergence; exact = every pass on all slices", true},
   {"keep", 0, true, "PCA on a subset of the samples: only those listed in this file (PLINK's --keep format: FID and IID are the first two fields of each line) enter the statistics and the eigenproblem; eigenvectors, pcs, --outload and --outmeansd are those of the subset, everyone else is projected onto its PCs (--outpcall)", true},
   {"remove", 0, true, "PCA on a subset of the samples: all but those listed in this file (same format; with --keep: keep first, then remove)", true},
   {"outpcall", 0, true, "PC output file for ALL samples in .fam order, in the format of the pcs file: the rows of the PCA's samples as in the pcs file, the samples left out by --keep / --remove projected onto the same PCs (written only when asked for)", true},
   {"accum", 0, true, "arithmetic of the two genotype GEMMs [auto | fp64 | fp32 | i8 | i8xS]: i8 = exact-integer int8 MFMA on S = 7 (i8xS: S = 2..8) byte slices of the fp64 operand, results equal to fp64; fp32 = fp32 MFMA products, fp64 long accumulation; auto (default) = i8, or fp64 if the int8 buffers do not fit", true},
};

// Long options like po::parse_command_line with its default style (flashpca.cpp:97; allow_guessing is part of
// command_line_style::default_style): the full name wins; otherwise an abbreviation that is a prefix of exactly one of the
// reference's options selects it (--nd 10, --outl f), and one that fits several is refused with boost's "ambiguous" error.
const OptSpec *find_long(const std::string &n, const std::string &as_typed)
{
   for (const auto &o : OPTS)
      if (n == o.name) return &o;
   std::vector<const OptSpec *> hits;
   if (!n.empty())
      for (const auto &o : OPTS)
         if (!o.ext && std::string(o.name).compare(0, n.size(), n) == 0) hits.push_back(&o);
   if (hits.size() == 1) return hits[0];
   if (hits.empty()) throw std::runtime_error("unrecognised option '" + as_typed + "'");
   std::string msg = "option '--" + n + "' is ambiguous and matches ";
   for (size_t i = 0; i < hits.size(); i++) {
      if (i) msg += i + 1 == hits.size() ? (hits.size() > 2 ? ", and " : " and ") : ", ";
      msg += std::string("'--") + hits[i]->name + "'";
   }
   throw std::runtime_error(msg);
}
const OptSpec *find_short(char c)
{
   for (const auto &o : OPTS)
      if (o.shortname && o.shortname == c) return &o;
   return nullptr;
}

template <class T, class Conv> T to_number(const VarMap &vm, const char *name, Conv conv)
{
   const std::string &s = vm.at(name);
   char *end = nullptr;
   errno = 0;
   T v = conv(s.c_str(), &end);
   if (*end != '\0' || errno != 0 || s.empty()) throw std::runtime_error(std::string("the argument ('") + s + "') for option '--" + name + "' is invalid");
   return v;
}
long to_long(const VarMap &vm, const char *name)
{
   return to_number<long>(vm, name, [](const char *s, char **end) { return std::strtol(s, end, 10); });
}
double to_double(const VarMap &vm, const char *name) { return to_number<double>(vm, name, std::strtod); }

} // namespace

VarMap parse_command_line(int argc, char *argv[])
{
   VarMap vm;
   for (int i = 1; i < argc; i++) {
      std::string a = argv[i];
      const OptSpec *o = nullptr;
      std::string val;
      bool have_val = false;
      if (a.rfind("--", 0) == 0) {
         std::string body = a.substr(2);
         size_t eq = body.find('=');
         if (eq != std::string::npos) {
            val = body.substr(eq + 1);
            have_val = true;
            body = body.substr(0, eq);
         }
         o = find_long(body, a);
      } else if (a.size() >= 2 && a[0] == '-') {
         o = find_short(a[1]);
         if (!o) throw std::runtime_error("unrecognised option '" + a + "'");
         if (a.size() > 2) {
            val = a.substr(2);
            have_val = true;
         }
      } else
         throw std::runtime_error("too many positional options have been specified on the command line");
      if (o->has_value) {
         if (!have_val) {
            if (i + 1 >= argc) throw std::runtime_error(std::string("the required argument for option '--") + o->name + "' is missing");
            val = argv[++i];
         }
         vm[o->name] = val;
      } else {
         if (have_val) throw std::runtime_error(std::string("option '--") + o->name + "' does not take any arguments");
         vm[o->name] = "";
      }
   }
   return vm;
}

void print_help()
{
   std::cerr << "Options:" << std::endl;
   for (const auto &o : OPTS) {
      std::string left = "  ";
      if (o.shortname) left += std::string("-") + o.shortname + " [ --" + o.name + " ]";
      else left += std::string("--") + o.name;
      if (o.has_value) left += " arg";
      while (left.size() < 30) left += ' ';
      std::cerr << left << " " << o.help << std::endl;
   }
   std::cerr << std::endl;
}

namespace {

typedef std::pair<const char *, int> Keyword; // word, value

// A keyword option: the value of the word given, or `dflt` without the option; any other word is refused with `unknown` in front
// of it.  --accum also takes i8xS: the int8 path on S = 2..8 byte slices.
int keyword(const VarMap &vm, const char *opt, int dflt, std::initializer_list<Keyword> words, const char *unknown)
{
   const auto it = vm.find(opt);
   if (it == vm.end()) return dflt;
   const std::string &m = it->second;
   for (const Keyword &k : words)
      if (m == k.first) return k.second;
   if (!std::strcmp(opt, "accum") && m.size() == 4 && m.compare(0, 3, "i8x") == 0 && m[3] >= '2' && m[3] <= '8') return FPCA_ACCUM_I8(m[3] - '0');
   throw UsageError(unknown + m);
}

std::string input_file(const VarMap &vm, const char *opt)
{
   if (vm.at(opt).empty()) throw UsageError(std::string("no file specified for --") + opt);
   return vm.at(opt);
}

} // namespace

Options validate(const VarMap &vm)
{
   auto has = [&](const char *n) { return vm.count(n) > 0; };
   auto text = [&](const char *n, const std::string &dflt) { return has(n) ? vm.at(n) : dflt; };
   auto number = [&](const char *n, long dflt) { return has(n) ? to_long(vm, n) : dflt; };
   Options o;
   o.verbose = has("verbose");

   // ---- mode selection (flashpca.cpp:136-228) ------------------------------------------------------------
   const char *modes[] = {"ucca", "scca", "check", "project"};
   for (const char *m1 : modes)
      for (const char *m2 : modes)
         if (std::string(m1) < m2 && has(m1) && has(m2))
            throw UsageError(std::string("conflicting modes requested: --") + m1 + ", --" + m2, true);
   if (has("scca")) throw UsageError("--scca is outside the PCA path this build implements");
   if (has("ucca")) o.mode = MODE_UCCA;
   else if (has("check")) o.mode = MODE_CHECK;
   else if (has("project")) {
      o.mode = MODE_PROJECT;
      if (!has("inload")) throw UsageError("SNP-loadings must be specified using --inload");
      if (!has("inmaf") && !has("inmeansd")) throw UsageError("one of MAF or mean/stdev must be specified using  --inmaf or --inmeansd, respectively");
   }

   if (has("memory") && to_long(vm, "memory") < 1) throw UsageError("memory (MB) must be >=1");
   if (has("blocksize")) {
      if (has("memory")) throw UsageError("cannot specify both --memory and --blocksize at the same time");
      if (to_long(vm, "blocksize") < 1) throw UsageError("blocksize must be >=1");
   }
   (void)number("numthreads", 0);
   o.seed = number("seed", 1L);

   if (!has("bfile") && !(has("bed") && has("bim") && has("fam"))) throw UsageError("you must specify either --bfile or --bed / --fam / --bim", true);
   o.geno_file = has("bfile") ? vm.at("bfile") + ".bed" : vm.at("bed");
   o.bim_file = has("bfile") ? vm.at("bfile") + ".bim" : vm.at("bim");
   o.fam_file = has("bfile") ? vm.at("bfile") + ".fam" : vm.at("fam");
   if (has("pheno")) // flashpca.cpp:316-322
      o.pheno_file = vm.at("pheno");
   else if (o.mode == MODE_UCCA)
      throw UsageError("you must specify a phenotype file in CCA/UCCA/SCCA mode using --pheno");

   o.n_dim = (int)number("ndim", 10);
   if (o.n_dim < 1) throw UsageError("--ndim can't be less than 1");
   o.stand_method_x = keyword(vm, "standx", FPCA_STANDARDISE_BINOM2, {{"binom", FPCA_STANDARDISE_BINOM}, {"binom2", FPCA_STANDARDISE_BINOM2}},
                              "unknown standardization method (--standx): ");
   if (o.mode == MODE_UCCA) // flashpca.cpp:352-372 (read in UCCA mode only: PCA has no phenotypes)
      o.stand_method_y = keyword(vm, "standy", FPCA_STANDARDISE_SD,
                                 {{"binom", FPCA_STANDARDISE_BINOM}, {"binom2", FPCA_STANDARDISE_BINOM2}, {"sd", FPCA_STANDARDISE_SD},
                                  {"center", FPCA_STANDARDISE_CENTER}, {"none", FPCA_STANDARDISE_NONE}},
                                 "unknown standardization method (--standy): ");
   const std::string suffix = text("suffix", ".txt");
   o.pcfile = text("outpc", "pcs" + suffix);
   o.eigvecfile = text("outvec", "eigenvectors" + suffix);
   o.eigvalfile = text("outval", "eigenvalues" + suffix);
   o.eigpvefile = text("outpve", "pve" + suffix);
   o.meansdfile = text("outmeansd", "meansd" + suffix);
   o.save_meansd = has("outmeansd");
   o.projfile = text("outproj", "projection" + suffix);
   o.uccafile = "ucca" + suffix; // flashpca.cpp:423

   o.maxiter = (int)number("maxiter", 500);
   if (o.maxiter <= 0) throw UsageError("--maxiter can't be less than 1");
   if (has("tol")) o.tol = to_double(vm, "tol");
   if (o.tol <= 0) throw UsageError("--tol can't be zero or negative");
   o.do_loadings = has("outload");
   o.loadingsfile = text("outload", "");
   o.divisor = keyword(vm, "div", FPCA_DIVISOR_P, {{"none", FPCA_DIVISOR_NONE}, {"n1", FPCA_DIVISOR_N1}, {"p", FPCA_DIVISOR_P}}, "unknown divisor (--div): ");
   if (has("inmeansd")) {
      if (has("inmaf")) throw UsageError("conflicting options requested --inmeansd, --inmaf");
      o.in_meansd_file = input_file(vm, "inmeansd");
   } else if (has("inmaf"))
      o.in_maf_file = input_file(vm, "inmaf");
   if (has("inload")) o.in_load_file = input_file(vm, "inload");
   o.precision = (int)number("precision", 7);
   if (o.precision <= 1) throw UsageError("output --precision too low");
   o.device = (int)number("device", 0);
   o.ngpus = (int)number("gpus", 1);
   if (o.ngpus < 1 || o.ngpus > 64) throw UsageError("--gpus must be between 1 and 64");
   if (o.ngpus > 1 && o.mode != MODE_PCA) throw UsageError("--gpus applies to PCA only (--ucca, --check and --project run on one GPU)");
   o.subset = has("keep") || has("remove");
   if (o.subset && (o.mode != MODE_PCA || o.ngpus > 1))
      throw UsageError("--keep / --remove apply to PCA on one GPU only (--check, --project, --ucca and --gpus run on all samples of the fileset)");
   o.keep_file = text("keep", "");
   o.remove_file = text("remove", "");
   if (has("outpcall") && o.mode != MODE_PCA) throw UsageError("--outpcall applies to PCA only");
   o.pcallfile = text("outpcall", "");
   o.blockvec = (int)number("blockvec", 0);
   o.maxblocks = (int)number("maxblocks", 0);
   o.accum = keyword(vm, "accum", FPCA_ACCUM_AUTO, {{"auto", FPCA_ACCUM_AUTO}, {"fp64", FPCA_ACCUM_FP64}, {"fp32", FPCA_ACCUM_FP32}, {"i8", FPCA_ACCUM_I8(7)}},
                     "unknown accumulate mode (--accum): ");
   o.replicated_solver = keyword(vm, "solver", 0, {{"rowshard", 0}, {"replicated", 1}}, "unknown --solver layout (rowshard | replicated): ");
   o.mixed = keyword(vm, "passes", 0, {{"mixed", 1}, {"exact", -1}}, "unknown --passes mode (mixed | exact): ");
   return o;
}

} // namespace cli
