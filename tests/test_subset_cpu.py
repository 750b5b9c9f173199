"""Sample subsets without a GPU: the two entry points in the header, the binding and both builds of the library; the --keep / --remove
id files (PLINK's format) and every refusal of the command line that is decided before device work, each with its exit code; the
abbreviations the reference accepts still mean what they meant; and the register discipline of the new kernels."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DATA = os.path.join(ROOT, "tests", "golden", "data_chr1")


def fam_ids():
    return [l.split()[:2] for l in open(DATA + ".fam").read().splitlines()]


def run(args, cwd):
    import flashpca_amd as fp

    return subprocess.run([fp.CLI_PATH] + args, capture_output=True, text=True, cwd=cwd, timeout=120)


def test_entry_points_declared_bound_and_exported(built_lib):
    import flashpca_amd as fp
    from flashpca_amd import _lib

    main = open(os.path.join(ROOT, "include", "fpca.h")).read()
    assert re.search(r"^int fpca_set_sample_mask\(fpca_ctx \*ctx, const uint8_t \*keep\);", main, re.M)
    assert re.search(r"^uint64_t fpca_nkept\(const fpca_ctx \*ctx\);", main, re.M)
    assert "#define FPCA_ABI_VERSION 4" in main  # (the mask is context state: no struct changed)
    for path in (fp.LIB_PATH, fp.HOOKS_LIB_PATH):
        L = C.CDLL(path)
        for name in ("fpca_set_sample_mask", "fpca_nkept"):
            assert name in _lib.SIGNATURES and getattr(L, name) is not None, (path, name)
    L = fp.lib()
    keep = np.ones(4, dtype=np.uint8)
    assert L.fpca_set_sample_mask(None, keep.ctypes.data_as(C.c_void_p)) == -1 and b"NULL context" in L.fpca_last_error()
    assert L.fpca_set_sample_mask(None, None) == -1
    assert L.fpca_nkept(None) == 0
    assert hasattr(fp.Context, "set_sample_mask") and isinstance(fp.Context.nkept, property)
    import inspect

    assert inspect.signature(fp.flashpca).parameters["keep"].default is None


def test_cli_subset_refusals_before_device_work(tmp_path, built_lib):
    ids = fam_ids()
    n = len(ids)
    assert n > 100

    def idfile(name, rows, extra=""):
        p = tmp_path / name
        p.write_text("".join("%s\t%s%s\n" % (a, b, extra) for a, b in rows))
        return str(p)

    k10 = idfile("k10.txt", ids[:10])
    base = ["--bfile", DATA, "--notime"]
    # a subset together with a mode that runs on all samples: refused in the style of "--gpus applies to PCA only"
    msg = "Error: --keep / --remove apply to PCA on one GPU only"
    for extra in (["--check"], ["--project", "--inload", "l.txt", "--inmeansd", "m.txt"], ["--ucca", "--pheno", "p.txt"], ["--gpus", "2"]):
        for flag in ("--keep", "--remove"):
            r = run(base + [flag, k10] + extra, tmp_path)
            assert r.returncode == 1 and msg in r.stderr, (extra, flag, r.stderr)
            assert "Start flashpca" not in r.stdout  # (refused while the command line is parsed)
    r = run(base + ["--outpcall", "all.txt", "--check"], tmp_path)
    assert r.returncode == 1 and "Error: --outpcall applies to PCA only" in r.stderr
    # the id files
    r = run(base + ["--keep", str(tmp_path / "nope.txt")], tmp_path)
    assert r.returncode == 1 and "Error reading file" in r.stderr and "nope.txt" in r.stderr
    r = run(base + ["--keep", idfile("unknown.txt", ids[:5] + [["NOFAM", "NOBODY"]])], tmp_path)
    assert r.returncode == 1 and "line 6: sample 'NOFAM NOBODY' is not in the .fam file" in r.stderr
    r = run(base + ["--remove", idfile("unknown2.txt", [[ids[0][0], "NOBODY"]])], tmp_path)
    assert r.returncode == 1 and "is not in the .fam file" in r.stderr
    one = tmp_path / "onefield.txt"
    one.write_text("%s %s\n%s\n" % (ids[0][0], ids[0][1], ids[1][0]))
    r = run(base + ["--keep", str(one)], tmp_path)
    assert r.returncode == 1 and "line 2: expected FID and IID, found one field" in r.stderr
    # fewer than two samples
    r = run(base + ["--keep", idfile("k1.txt", ids[:1])], tmp_path)
    assert r.returncode == 1 and "Error: --keep / --remove leave 1 of %d samples, at least 2 are needed" % n in r.stderr
    r = run(base + ["--remove", idfile("rall.txt", ids)], tmp_path)
    assert r.returncode == 1 and "leave 0 of %d samples" % n in r.stderr
    r = run(base + ["--keep", idfile("k3.txt", ids[:3]), "--remove", idfile("r2.txt", ids[1:3])], tmp_path)
    assert r.returncode == 1 and "leave 1 of %d samples" % n in r.stderr
    # What the lists select is visible without a device through the dimension limit (min(n_kept, P) - 1) / 2, refused before the upload.
    # Five samples: ndim 2 at most.  Duplicate lines, further fields, blank lines, spaces or tabs and a last line without a newline are harmless.
    five = tmp_path / "five.txt"
    rows = ids[:5] + ids[:3]
    five.write_text("\n".join("%s %s\textra 1 2" % (a, b) for a, b in rows[:4]) + "\n\n   \n" + "\n".join("%s\t%s" % (a, b) for a, b in rows[4:]))
    r = run(base + ["--keep", str(five), "--ndim", "3"], tmp_path)
    assert r.returncode == 1 and "Error: You asked for 3 dimensions, but only 2allowed" in r.stderr, r.stderr
    # keep first, then remove: 9 - 2 = 7 samples allow 3 dimensions, not 4
    k9, r2 = idfile("k9.txt", ids[20:29]), idfile("r2b.txt", ids[27:31])  # (two of the four removed ids are among the kept)
    r = run(base + ["--keep", k9, "--remove", r2, "--ndim", "4"], tmp_path)
    assert r.returncode == 1 and "You asked for 4 dimensions, but only 3allowed" in r.stderr, r.stderr
    # --remove alone: n - 4 samples
    r = run(base + ["--remove", r2, "--ndim", str((n - 4 - 1) // 2 + 1)], tmp_path)
    assert r.returncode == 1 and "but only %dallowed" % ((n - 4 - 1) // 2) in r.stderr, r.stderr
    # without a subset the limit is that of all samples, as before
    r = run(base + ["--ndim", str((n - 1) // 2 + 1)], tmp_path)
    assert r.returncode == 1 and "but only %dallowed" % ((n - 1) // 2) in r.stderr


def test_reference_abbreviations_keep_their_meaning(tmp_path, built_lib):
    """The new flags are matched by their full names only: --outp stays ambiguous between the reference's five options (--outpcall is
    not among them), --outpc is the PC output file, and no prefix selects a new flag."""
    base = ["--bfile", DATA, "--notime"]
    r = run(base + ["--outp", "x"], tmp_path)
    assert "option '--outp' is ambiguous and matches '--outpc', '--outpcx', '--outpcy', '--outpve', and '--outproj'" in r.stderr
    r = run(base + ["--outpc", "x", "--nd", "0"], tmp_path)
    assert "--ndim can't be less than 1" in r.stderr
    for abbrev in ("--kee", "--remov", "--outpca", "--outpcal"):
        r = run(base + [abbrev, "x"], tmp_path)
        assert "unrecognised option '%s'" % abbrev in r.stderr and "Start flashpca" not in r.stdout, (abbrev, r.stderr)
    r = run(["--help"], tmp_path)
    for flag in ("--keep arg", "--remove arg", "--outpcall arg"):
        assert flag in r.stderr


def test_subset_kernels_do_not_spill():
    """The pattern of tests/test_scca_cv_cpu.py: no kernel of sample_mask.hip may compile with spills, by the compiler's own remarks
    (-Rpass-analysis=kernel-resource-usage) and by the code object's metadata."""
    csrc = os.path.join(ROOT, "flashpca_amd", "csrc")
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "sample_mask.s")
        r = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S",
                            "-Rpass-analysis=kernel-resource-usage", os.path.join(csrc, "sample_mask.hip"), "-o", out], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        txt = open(out).read()
    names = re.findall(r"\.name:\s+(\S+)", txt)
    spills = re.findall(r"\.vgpr_spill_count:\s+(\d+)", txt)
    sspills = re.findall(r"\.sgpr_spill_count:\s+(\d+)", txt)
    assert len(names) == len(spills) == len(sspills) and names
    for k in ("k_bed_stats_masked", "k_mask_rows", "k_gather_kept", "k_scatter_kept"):
        assert any(k in n for n in names), k
    assert all(int(s) == 0 for s in spills + sspills), list(zip(names, spills, sspills))
    remarks = re.findall(r"remark:\s+(VGPRs|SGPRs) Spill: (\d+)", r.stderr)
    assert len(remarks) == 2 * len(names) and all(int(v) == 0 for _, v in remarks), remarks
    # the statistics kernel is a kernel of its own: K1 and the fold counts are not touched by it
    src = open(os.path.join(csrc, "sample_mask.hip")).read()
    assert "k_bed_stats_masked" in src and "k_bed_stats_masked" not in open(os.path.join(csrc, "kernels.hip")).read()
