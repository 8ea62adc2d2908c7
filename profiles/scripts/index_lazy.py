"""The index kernels that profiles/scripts/index_alone.py (the index plan) does not reach, on one mid-size level (2 x [21, 400, 352], 80 k
sites), 20 times: from_coords (gi_mark_coords, the three-kernel scan, gi_rowof), from_conv (gi_mark_conv, scan, gi_decode), the generic
SubM / conv table kernels and the scattered o2i arm of rb_conv_kernel.  Run under `rocprofv3 --kernel-trace --stats` for the per-kernel
durations (profiles/grid_index_shared_ab.txt)."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import helpers as H  # noqa: E402
from toda_amd import lib, ops  # noqa: E402

print("library", lib.LIB_PATH, flush=True)
BATCH, SHAPE = 2, [21, 400, 352]
sites, _ = H.clustered_sparse(BATCH, SHAPE, 40000, 1, seed=3)
idx = torch.as_tensor(np.ascontiguousarray(sites)).cuda()
print("sites", len(sites), flush=True)
for it in range(20):
    gi = ops.GridIndex.from_coords(idx, BATCH, SHAPE)
    ops.build_subm_rulebook(idx, BATCH, SHAPE, (5, 5, 1), (1, 1, 1), grid_index=gi)
    ops.build_subm_rulebook(idx, BATCH, SHAPE, (3, 3, 3), (1, 1, 1), grid_index=gi)
    ops.build_conv_rulebook(idx, BATCH, SHAPE, (3, 3, 3), (2, 2, 2), (1, 1, 1))
    ops.build_conv_rulebook(idx, BATCH, SHAPE, (2, 2, 2), (2, 2, 2), (0, 0, 0))
    ops.build_conv_rulebook(idx, BATCH, SHAPE, (3, 1, 1), (2, 1, 1), (0, 0, 0))
    torch.cuda.synchronize()
print("done", flush=True)
