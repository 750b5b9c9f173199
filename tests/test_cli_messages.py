"""What the flashpca CLI answers before any device work: parse errors, --version / --help, every usage refusal, the checks made
from the text files and the file sizes, and pairs of faulty options that pin the ORDER of the checks (the first failing one decides
the message).  tests/golden/cli_messages.json holds, for each command line, the exit status, stdout and stderr that the build BEFORE
the CLI was split into cli_options / cli_multi / cli_main gave (all with --notime where the arguments line is printed); the built
CLI must give the same bytes.  In the fixture {CLI} stands for the binary, {DATA} for tests/golden/data_chr1, {VERSION} for
FPCA_VERSION of include/fpca.h and {TMP} for the working directory, where the small files below are written.  The fixture is a
record: it is not to be regenerated from a newer binary."""
import json
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "flashpca_amd", "_build", "flashpca")
VERSION = re.search(r'#define FPCA_VERSION "([^"]+)"', open(os.path.join(ROOT, "include", "fpca.h")).read()).group(1)
DATA = os.path.join(ROOT, "tests", "golden", "data_chr1")
CASES = json.load(open(os.path.join(ROOT, "tests", "golden", "cli_messages.json")))


def write_small_files(tmp):
    """The inputs of the file checks: a .bim that is 7 SNPs short, a --keep list of one sample, a phenotype file of 5 rows,
    and a 3-sample .fam with a 2-phenotype file (UCCA admits N - 2 = 1 there)."""
    fam = open(DATA + ".fam").read().splitlines(True)
    bim = open(DATA + ".bim").read().splitlines(True)
    open(os.path.join(tmp, "short.bim"), "w").writelines(bim[:-7])
    open(os.path.join(tmp, "keep1.txt"), "w").write(" ".join(fam[0].split()[:2]) + "\n")
    open(os.path.join(tmp, "pheno5.txt"), "w").writelines("%s 0.5\n" % " ".join(l.split()[:2]) for l in fam[:5])
    open(os.path.join(tmp, "three.fam"), "w").writelines(fam[:3])
    open(os.path.join(tmp, "pheno3x2.txt"), "w").writelines("%s 0.5 1.5\n" % " ".join(l.split()[:2]) for l in fam[:3])


def fill(text, tmp):
    return text.replace("{TMP}", str(tmp)).replace("{DATA}", DATA).replace("{CLI}", CLI).replace("{VERSION}", VERSION)


def run_case(argv, tmp):
    write_small_files(str(tmp))
    return subprocess.run([CLI] + [fill(a, tmp) for a in argv], capture_output=True, text=True, cwd=str(tmp), timeout=120)


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_cli_message(case, tmp_path, built_lib):
    r = run_case(case["argv"], tmp_path)
    assert r.returncode == case["status"], (case["argv"], r.stderr)
    assert r.stderr == fill(case["stderr"], tmp_path), case["argv"]
    assert r.stdout == fill(case["stdout"], tmp_path), case["argv"]
