"""Records gru_sweep_parent_counts.npz: the counters of npd_gru_decode_count_sweep on the pinned cases of
tests/test_gru_sweep_strip_gpu.py, from this project's own kernel.  Run on the GPU at the commit whose counters are to
be pinned (the one before gru16p_kernel's step loop changed):  python tests/golden/gen_gru_sweep_parent.py [out.npz]"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))            # tests/ (conftest, the test module)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import test_gru_sweep_strip_gpu as T  # noqa: E402

out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "gru_sweep_parent_counts.npz")
counts = {name: T.sweep_counts(name) for name in T.PINNED}
for k, v in counts.items():
    print(k, v.tolist())
np.savez(out, **counts)
