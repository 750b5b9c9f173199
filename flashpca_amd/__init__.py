"""flashpca_amd -- MI355X-native implementation of flashpca's PCA hot path (its per-SNP UCCA scan and sparse CCA).

The product is the C-ABI library flashpca_amd/_build/libfpca.so (include/fpca.h; hand-written gfx950 HIP kernels
+ C++ host eigensolver) and the drop-in `flashpca` CLI next to it.  This package is the thin Python mirror used
by tests and bench.py.  There is no CPU fallback.
"""
from ._lib import LIB_PATH, CLI_PATH, HOOKS_LIB_PATH, HOOKS_CLI_PATH, build, lib, test_hooks, FpcaError  # noqa: F401
from .api import Context, flashpca, project, ucca, scca, cv_scca, snp_filter, ld_prune, king_cutoff, qc_filter, count_fam_rows  # noqa: F401
from .api import king_related, king_classify, write_kin0  # noqa: F401
from .api import grm, rel_cutoff, write_grm, read_grm  # noqa: F401
from .api import pcrelate  # noqa: F401
from .api import pcrelate_ibd, pcrelate_related, pcrelate_classify  # noqa: F401
from .api import pcair, pcair_partition, pcair_partition_rule  # noqa: F401
from .api import debug_synth_host  # noqa: F401
from .api import check_pca as check  # noqa: F401  (R: check())

__version__ = "0.1.0"
