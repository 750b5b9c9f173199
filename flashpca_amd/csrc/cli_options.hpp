// cli_options.hpp -- the command line of `flashpca`: the option table and its boost-style parser, and the validated Options
// every later step reads.  Pure host C++: nothing here touches the device; of include/fpca.h only the constants are used.
#pragma once
#include <map>
#include <stdexcept>
#include <string>

#include "../../include/fpca.h"

#define FLASHPCA_VERSION "2.1-mi355x (" FPCA_VERSION ")"

namespace cli {

extern bool show_timestamp; // false under --notime
std::string timestamp();    // "[Thu Jan  1 00:00:00 1970] " or "" (util.cpp:270-283)

// A refusal of the command line or of the input files' sizes: main() prints "Error: <message>" [, "Use --help to get more help"]
struct UsageError : std::runtime_error {
   bool with_help_hint;
   explicit UsageError(const std::string &message, bool hint = false) : std::runtime_error(message), with_help_hint(hint) {}
};

typedef std::map<std::string, std::string> VarMap;

// throws std::runtime_error like boost::program_options does on malformed command lines
VarMap parse_command_line(int argc, char *argv[]);
void print_help();

enum Mode { MODE_PCA, MODE_CHECK, MODE_PROJECT, MODE_UCCA };

struct Options {
   Mode mode = MODE_PCA;
   bool verbose = false;
   std::string geno_file, bim_file, fam_file, pheno_file;
   int n_dim = 10, stand_method_x = FPCA_STANDARDISE_BINOM2, stand_method_y = FPCA_STANDARDISE_SD, divisor = FPCA_DIVISOR_P;
   int maxiter = 500, precision = 7;
   double tol = 1e-6;
   long seed = 1;
   int device = 0, ngpus = 1, blockvec = 0, maxblocks = 0, accum = FPCA_ACCUM_AUTO, mixed = 0, replicated_solver = 0;
   std::string pcfile, eigvecfile, eigvalfile, eigpvefile, meansdfile, projfile, uccafile, loadingsfile, pcallfile;
   bool do_loadings = false, save_meansd = false;
   std::string in_meansd_file, in_maf_file, in_load_file;
   bool subset = false; // --keep and / or --remove
   std::string keep_file, remove_file;
};

// flashpca.cpp:136-560: the reference's checks and this build's own, in the reference's order (the first that fails decides the
// message).  Throws UsageError; a malformed number is a std::runtime_error worded like boost's.
Options validate(const VarMap &vm);

} // namespace cli
