"""The roofline table's cost functions (bench.py --layers) read each call's arguments by the parameter names of
include/toda.h.  Every wrapped entry point is priced here from an argument tuple whose position i holds 100 + i, so a
name that resolves to another position changes the key or the cost.  The expected values were recorded from the cost
functions as they were while they still indexed the tuple by position.  No GPU and no patched module: the functions are
called on the class."""
import pytest

from toda_amd import lib as L
from toda_amd.tools.op_table import OpTable

# the host arrays that three cost functions dereference: entry point -> {position: values}
HOST_ARRAYS = {
    "toda_voxelize_batch": {1: [50 + 3 * j for j in range(102)]},          # n_points_host[batch], batch = 100 + 2
    "toda_gridindex_from_bitmap": {2: [41, 160, 176], 6: [21, 80, 88]},      # shape_in_host, shape_out_host
    "toda_sparse_to_dense_fwd": {5: [2, 20, 22]},                            # shape_host
    "toda_sparse_to_dense_bwd": {5: [2, 20, 22]},
}

EXPECTED = {
    "toda_bn2d_bwd": ((102, 103, 104), ("fixed", 13111488.0, 0.0, "x once, dy once, dx once")),
    "toda_bn2d_bwd_from": ((104, 105, 106, 102), ("fixed", 13890240.0, 0.0, "x once, dy (a channel slice) once, dx once")),
    "toda_bn2d_fwd": ((101, 102, 103), ("fixed", 8488848.0, 0.0, "x read once, y written once")),
    "toda_bn2d_fwd_into": ((101, 102, 103, 112), ("fixed", 8488848.0, 0.0, "x read once, y written once into its channel slice of the concatenated map")),
    "toda_center_assign": ((), ("fixed", 0.0, 0.0, "latency bound")),
    "toda_clip_adam_step": ((107,), ("fixed", 31555584.0, 0.0, "g twice, p / m / v read and written, g written: 36 bytes per parameter (upper bound: whole chunks)")),
    "toda_conv3x3_transform_weight": ((101, 102, 103), ("fixed", 1854360.0, 0.0, "")),
    "toda_conv3x3s2_dgrad": ((102, 103, 104, 105, 106, 2), ("fixed", 585055344.0, 54202891392.0, "")),
    "toda_conv3x3s2_fwd": ((102, 103, 104, 105, 106, 2), ("fixed", 585055344.0, 54202891392.0, "")),
    "toda_conv3x3s2_wgrad": ((102, 103, 104, 105, 106, 2), ("fixed", 585055344.0, 54202891392.0, "")),
    "toda_deconv_dgrad": ((102, 103, 104, 105, 106, 107), ("fixed", 5407956457712.0, 278460405437760.0, "")),
    "toda_deconv_fwd": ((102, 103, 104, 105, 106, 107), ("fixed", 5407956457712.0, 278460405437760.0, "")),
    "toda_deconv_wgrad": ((102, 103, 104, 105, 106, 107), ("fixed", 5407956457712.0, 278460405437760.0, "")),
    "toda_gridindex_clear": ((101,), ("fixed", 2424.0, 0.0, "16 B coordinate row + one 8-byte cell per site; n = upper bound (cap) of the rows")),
    "toda_gridindex_from_bitmap": ((101, 21, 80, 88), ("fixed", 32885600.0, 0.0, "one pass over the input bitmap's and the output bitmap's 8-byte words (output rows not counted)")),
    "toda_gridindex_from_conv": ((101,), ("fixed", 3232.0, 0.0, "16 B in + 16 B out per site (upper bound on N_out = N_in)")),
    "toda_gridindex_from_coords": ((101,), ("fixed", 2424.0, 0.0, "16 B coordinate row + one 8-byte cell per site (bitmap clear / scan not counted)")),
    "toda_gridindex_from_coords_unordered": ((101,), ("fixed", 2424.0, 0.0, "16 B coordinate row + one 8-byte cell per site; n = upper bound (cap) of the rows")),
    "toda_mean_vfe_bwd": ((102, 103, 104), ("fixed", 4413336.0, 0.0, "")),
    "toda_mean_vfe_fwd": ((102, 103, 104), ("fixed", 4413336.0, 0.0, "")),
    "toda_rows_affine_act": ((104, 105), ("fixed", 131040.0, 0.0, "")),
    "toda_rows_bn_bwd_res": ((105, 106), ("fixed", 222600.0, 0.0, "")),
    "toda_rows_moments": ((101, 102), ("fixed", 41208.0, 0.0, "")),
    "toda_rulebook_class_order": ((101,), ("fixed", 2121.0, 0.0, "16 B coordinate row in, order + class out")),
    "toda_rulebook_conv": ((101, 109), ("fixed", 26040.0, 0.0, "both tables (o2i, i2o)")),
    "toda_rulebook_subm": ((101,), ("fixed", 14140.0, 0.0, "16 N_in + 16 N_out + the 27 x N table it writes")),
    "toda_sparse_to_dense_bwd": ((102, 103, 104, 2, 20, 22), ("fixed", 37748264.0, 0.0, "sparse rows + the dense map")),
    "toda_sparse_to_dense_fwd": ((102, 103, 104, 2, 20, 22), ("fixed", 37748264.0, 0.0, "sparse rows + the dense map")),
    "toda_spconv_pack_weight": ((101, 102, 103), ("fixed", 8488848.0, 0.0, "")),
    "toda_voxelize_batch": ((102, 20553, 104, 109), ("fixed", 969147768.0, 0.0, "whole batch (3 launches): per sample 4NC + 8MPC + 20M, M bounded by min(cap, points)")),
    "toda_voxelize_hard": ((101, 102, 106), ("fixed", 8779324.0, 0.0, "M bounded by min(cap, points)")),
}


def arguments(name):
    args = [100 + i for i in range(len(L.SIGNATURES[name][1]))]
    keep = []
    for pos, vals in HOST_ARRAYS.get(name, {}).items():
        keep.append(L.host_i32(vals))
        args[pos] = L.hptr(keep[-1])
    return tuple(args), keep


@pytest.mark.parametrize("name", sorted(EXPECTED))
def test_cost_of_a_call_by_header_names(name):
    args, keep = arguments(name)
    assert OpTable.cost_of(name, args) == EXPECTED[name]


def test_every_cost_function_is_covered():
    assert sorted(a[3:] for a in vars(OpTable) if a.startswith("_c_toda_")) == sorted(EXPECTED)
    assert set(EXPECTED) <= set(L.ARG_NAMES)
