"""CPU test: bench.py's dump_outputs on a small host tensor, the whole-product branch and the seeded row sample the headline size
takes.  torch is imported in a child process only: it brings its own HIP runtime and librccl, which would shadow the system RCCL
for the GPU tests that share a pytest process with this one."""
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = """
import sys
import torch
import bench
N, b, rows, out = 50, 4, 64, sys.argv[1]
Y = torch.arange(rows * b, dtype=torch.float64).reshape(rows, b)  # row r holds r b ... r b + b - 1; rows >= N are padding
bench.dump_outputs(out + "/whole", Y, N, b)
bench.DUMP_MAX_VALUES = 16 * b + 3  # 16 rows
bench.dump_outputs(out + "/sample1", Y, N, b)
bench.dump_outputs(out + "/sample2", Y, N, b)
"""


def test_dump_outputs_whole_and_sampled(tmp_path):
    subprocess.run([sys.executable, "-c", CHILD, str(tmp_path)], check=True, timeout=300, cwd=ROOT,
                   env=dict(os.environ, PYTHONPATH=ROOT))
    N, b = 50, 4
    whole = np.load(tmp_path / "whole" / "Y.npy")
    assert whole.dtype == np.float64 and np.array_equal(whole, np.arange(N * b, dtype=np.float64).reshape(N, b))
    s1, s2 = np.load(tmp_path / "sample1" / "Y.npy"), np.load(tmp_path / "sample2" / "Y.npy")
    assert s1.dtype == np.float64 and s1.shape == (16, b) and np.array_equal(s1, s2)  # fixed seed: the same rows every time
    idx = (s1[:, 0] / b).astype(int)
    assert np.all(np.diff(idx) > 0) and idx[-1] < N  # distinct rows in ascending order, none of the padding
    assert np.array_equal(s1, whole[idx])  # each sampled row whole and unchanged
