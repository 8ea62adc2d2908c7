"""The grid index and rulebook builders of csrc/rulebook.hip without a GPU: the C oracle (O.rulebook_subm, O.rulebook_conv) against
the plain reference of tests/rulebook_cases.py on every case that test_gpu_rulebook_edges.py uses, the case tables against the
branches they are meant for, the buffer layout against toda_gridindex_bytes, and the argument checks that return -1 with a message
before anything is launched or dereferenced."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import rulebook_cases as RC
from toda_amd import lib as L

FAKE = 4096        # a non-null "device pointer" for arguments a refused call must not touch


def refused(rc, *words):
    msg = L.load().toda_last_error().decode()
    return rc == -1 and all(w in msg for w in words)


def same_conv(idx, batch, shape, ks, st, pd):
    io0, sho0, o2i0, i2o0, cnt0 = O.rulebook_conv(idx, batch, list(shape), ks, st, pd)
    io1, sho1, o2i1, i2o1, cnt1 = RC.conv_reference(idx, batch, shape, ks, st, pd)
    assert sho0 == sho1
    assert np.array_equal(io0, io1) and np.array_equal(o2i0, o2i1) and np.array_equal(i2o0, i2o1) and np.array_equal(cnt0, cnt1)
    assert int(cnt1.sum()) == int((i2o1 >= 0).sum()) == int((o2i1 >= 0).sum())
    return io1


def same_subm(idx, batch, shape, ks, dil):
    nbr0, cnt0 = O.rulebook_subm(idx, batch, list(shape), ks, dil)
    nbr1, cnt1 = RC.subm_reference(idx, batch, shape, ks, dil)
    assert np.array_equal(nbr0, nbr1) and np.array_equal(cnt0, cnt1)
    return nbr1


# ------------------------------------------------------------------------------- the two references agree
@pytest.mark.parametrize("g,l", RC.STRIDED_CASES, ids=[RC.geom_id(g) + "-" + RC.lattice_id(l) for g, l in RC.STRIDED_CASES])
def test_oracle_equals_the_plain_reference_on_the_strided_geometries(g, l):
    (shape, batch), (ks, st, pd) = RC.LATTICES[l], RC.STRIDED_GEOMS[g]
    for idx in RC.strided_sites(l):
        same_conv(idx, batch, shape, ks, st, pd)


@pytest.mark.parametrize("name", RC.OCCUPANCY_NAMES)
def test_oracle_equals_the_plain_reference_on_the_occupancy_sets(name):
    batch, shape, orders = RC.occupancy_sets()[name]
    for idx in orders:
        for ks, dil in RC.SUBM_KERNELS:
            same_subm(idx, batch, shape, ks, dil)
        io = same_conv(idx, batch, shape, *RC.OCC_CONV)
        same_subm(io, batch, RC.conv_out_shape(shape, *RC.OCC_CONV), (3, 3, 3), (1, 1, 1))


def test_oracle_equals_the_plain_reference_on_the_large_lattices():
    for sites, batch, shape, geom in ((RC.carry_sites(), RC.CARRY_BATCH, RC.CARRY_SHAPE, RC.CARRY_CONV),
                                      (RC.big_sites(), RC.BIG_BATCH, RC.BIG_SHAPE, RC.BIG_CONV)):
        for idx in sites:
            same_subm(idx, batch, shape, (3, 3, 3), (1, 1, 1))
            same_conv(idx, batch, shape, *geom)
    same_conv(RC.strided_sites(1)[1], RC.LATTICES[1][1], RC.LATTICES[1][0], *RC.TOO_WIDE)


def test_plain_reference_on_a_set_small_enough_to_write_down():
    """[1, 1, 6] with sites at x = 0, 1, 5, rows given as (5, 0, 1): k = 3, s = 2, p = 1 has the outputs x = 0 (window -1..1), 1 (1..3)
    and 2 (3..5)"""
    idx = np.array([[0, 0, 0, 5], [0, 0, 0, 0], [0, 0, 0, 1]], np.int32)
    io, sho, o2i, i2o, cnt = RC.conv_reference(idx, 1, (1, 1, 6), (1, 1, 3), (1, 1, 2), (0, 0, 1))
    assert sho == [1, 1, 3] and io.tolist() == [[0, 0, 0, 0], [0, 0, 0, 1], [0, 0, 0, 2]]
    assert o2i.tolist() == [[-1, 2, -1], [1, -1, -1], [2, -1, 0]]
    assert i2o.tolist() == [[-1, -1, 1], [-1, 0, -1], [2, -1, 0]] and cnt.tolist() == [1, 1, 2]
    nbr, cnt = RC.subm_reference(idx, 1, (1, 1, 6), (1, 1, 3), (1, 1, 1))
    assert nbr.tolist() == [[-1, -1, 1], [0, 1, 2], [-1, 2, -1]] and cnt.tolist() == [1, 3, 1]
    # a neighbour at x - 1 of x = 0 is not the previous row's last cell
    idx = np.array([[0, 0, 0, 2], [0, 0, 1, 0]], np.int32)
    nbr, _ = RC.subm_reference(idx, 1, (1, 2, 3), (1, 1, 3), (1, 1, 1))
    assert nbr.tolist() == [[-1, -1], [0, 1], [-1, -1]]


# ------------------------------------------------------------------------------- the case tables reach their branches
def test_left_out_combinations_are_exactly_those_without_an_output_cell():
    empty = [(g, l) for g, (ks, st, pd) in enumerate(RC.STRIDED_GEOMS) for l, (shape, _) in enumerate(RC.LATTICES)
             if min(RC.conv_out_shape(shape, ks, st, pd)) < 1]
    assert empty == RC.EMPTY_OUTPUT
    for g, l in empty:
        assert any(s + 2 * p < k for s, k, p in zip(RC.LATTICES[l][0], RC.STRIDED_GEOMS[g][0], RC.STRIDED_GEOMS[g][2]))
    assert len(RC.STRIDED_CASES) == len(RC.STRIDED_GEOMS) * len(RC.LATTICES) - len(RC.EMPTY_OUTPUT)


def test_strided_geometries_reach_both_arms_of_the_output_set_kernel():
    arm = ["per-bit" if st[2] > 2 or ks[2] > 8 else "shift-or" for ks, st, _ in RC.STRIDED_GEOMS]
    assert arm.count("per-bit") >= 3 and arm.count("shift-or") >= 4
    assert any(st[2] == 1 and ks[2] == 3 for ks, st, _ in RC.STRIDED_GEOMS)                  # stride 1 that is no copy
    assert any(ks[0] * ks[1] * ks[2] == 64 for ks, _, _ in RC.STRIDED_GEOMS)
    assert all(31 * st[2] + ks[2] <= 128 for ks, st, _ in RC.STRIDED_GEOMS) and any(31 * st[2] + ks[2] == 128 for ks, st, _ in RC.STRIDED_GEOMS)
    assert 31 * RC.TOO_WIDE[1][2] + RC.TOO_WIDE[0][2] == 129
    assert any(pd[2] > 0 for _, _, pd in RC.STRIDED_GEOMS)                                   # windows that start left of the row
    # none of them is one of the specialised 3x3x3 / 3x1x1 stride-2 layers' only shapes: the generic table kernel runs
    assert sum(1 for ks, _, _ in RC.STRIDED_GEOMS if tuple(ks) not in ((3, 3, 3), (3, 1, 1))) >= 6
    widths = [shape[2] for shape, _ in RC.LATTICES]
    assert 1 in widths and any(1 < w < 32 and w % 32 not in (0, 31) for w in widths) and 31 in widths and 65 in widths and 64 in widths


def test_occupancy_sets_hold_what_their_names_say():
    sets = RC.occupancy_sets()
    assert sorted(sets) == sorted(RC.OCCUPANCY_NAMES)
    for name, (batch, shape, (canon, shuf)) in sets.items():
        keys = RC.lin_keys(canon, shape)
        assert np.all(np.diff(keys) > 0) and RC.in_lattice(canon, batch, shape).all()
        assert sorted(map(tuple, shuf.tolist())) == sorted(map(tuple, canon.tolist()))
        assert len(canon) < 2 or not np.array_equal(canon, shuf)
        lay = RC.Layout(batch, shape)
        words = RC.bitmap_words(canon, batch, shape)
        if name.startswith("full"):
            assert len(canon) == lay.bits and (words[:lay.bits // 32] == 0xFFFFFFFF).all()
        if name == "first-cell":
            assert canon.tolist() == [[0, 0, 0, 0]] and words[0] == 1
        if name == "last-cell":
            assert keys.tolist() == [lay.bits - 1]
        if name == "no-site":
            assert canon.shape == (0, 4) and canon.dtype == np.int32
        if "empty" in name:
            assert len(set(canon[:, 0].tolist())) == batch - 1
        if name.startswith("faces"):
            hi = np.asarray(shape) - 1
            assert np.all(np.any((canon[:, 1:] == 0) | (canon[:, 1:] == hi), axis=1))
            corners = {(b, z, y, x) for b in range(batch) for z in (0, hi[0]) for y in (0, hi[1]) for x in (0, hi[2])}
            assert corners <= set(map(tuple, canon.tolist()))
    # the faces of 7 x 9 x 64 leave rows with sites at x = 0 and x = 63 only: output bit 31 of a stride-2 row then hangs on window bit 64
    canon = sets["faces-7x9x64x1"][2][0]
    assert sorted(canon[(canon[:, 1] == 2) & (canon[:, 2] == 3), 3].tolist()) == [0, 63]


def test_large_lattices_sit_just_above_their_thresholds():
    lay = RC.Layout(RC.CARRY_BATCH, RC.CARRY_SHAPE)
    assert 256 < -(-lay.cells // 2048) <= 264                       # the scan's partials need a second round of 256, and little more
    canon, _ = RC.carry_sites()
    keys = RC.lin_keys(canon, RC.CARRY_SHAPE)
    assert keys[0] == 0 and keys[-1] == lay.bits - 1 and (keys >> 5 >= 256 * 2048).sum() > 100 and (keys >> 5 < 2048).sum() > 100
    assert 1500 < len(canon) < 6000
    assert RC.conv_out_shape(RC.CARRY_SHAPE, *RC.CARRY_CONV) == list(RC.CARRY_SHAPE)

    lay = RC.Layout(RC.BIG_BATCH, RC.BIG_SHAPE)
    assert 2 ** 31 < lay.bits < 2 ** 31 + 2 ** 20 and lay.cells >= 2 ** 26 and lay.bits < 2 ** 36
    assert RC.conv_out_shape(RC.BIG_SHAPE, *RC.BIG_CONV) == list(RC.BIG_SHAPE)
    canon, _ = RC.big_sites()
    keys = RC.lin_keys(canon, RC.BIG_SHAPE)
    assert keys[0] == 0 and keys[-1] == lay.bits - 1 and 1500 < len(canon) < 6000
    assert {2 ** 31 - 1, 2 ** 31, 2 ** 31 + 1} <= set(keys.tolist())
    assert (keys < 2 ** 31).sum() > 500 and (keys >= 2 ** 31).sum() > 500
    assert lay.bytes < 0.56e9


# ------------------------------------------------------------------------------- buffer layout
def test_layout_matches_the_size_query():
    lib = L.load()
    for shape, batch in RC.LATTICES + [(RC.CARRY_SHAPE, RC.CARRY_BATCH), (RC.BIG_SHAPE, RC.BIG_BATCH), ((3, 4, 33), 2), ((41, 1600, 1408), 2)]:
        lay = RC.Layout(batch, shape)
        assert lib.toda_gridindex_bytes(batch, L.hptr(L.host_i32(shape))) == lay.bytes
        assert lay.o_part >= lay.cells * 8 and lay.o_rows % 256 == 0 and lay.bytes - lay.o_rows >= lay.rows


def test_bitmap_helpers_agree_with_a_loop():
    shape, batch = (3, 4, 31), 2
    canon, shuf = RC.strided_sites(2)
    cells = RC.canonical_cells(shuf, batch, shape)
    keys = RC.lin_keys(canon, shape)
    for r, k in enumerate(keys.tolist()):
        assert cells[k >> 5, 0] >> (k & 31) & 1
    assert int(RC.popcount32(cells[:, 0]).sum()) == len(canon)
    assert np.array_equal(RC.ranks(cells, keys), np.arange(len(canon)))
    free = np.setdiff1d(np.arange(RC.Layout(batch, shape).bits), keys)
    assert (RC.ranks(cells, free) == -1).all()
    rb = RC.row_bytes(shuf, batch, shape)
    assert set(np.flatnonzero(rb).tolist()) == {(b * shape[0] + z) * shape[1] + y for b, z, y, _ in canon.tolist()}


# ------------------------------------------------------------------------------- argument checks
def h3(v):
    return L.hptr(L.host_i32(v))


def test_subm_refuses_large_and_even_kernels_before_it_launches():
    lib = L.load()
    for ks, word in RC.REFUSED_SUBM:
        rc = lib.toda_rulebook_subm(FAKE, 10, 1, h3((8, 8, 8)), h3(ks), h3((1, 1, 1)), FAKE, None, FAKE, FAKE, 1, None)
        assert refused(rc, "rulebook_subm", word), (ks, L.last_error())
    rc = lib.toda_rulebook_subm(FAKE, 10, 1, h3((8, 8, 8)), h3((3, 3, 3)), h3((1, 0, 1)), FAKE, None, FAKE, FAKE, 1, None)
    assert refused(rc, "rulebook_subm", "dilation")


def conv_calls(lib, shape, ks, st, pd, sho):
    """the three entry points that take a strided geometry, with pointers a refused call must not touch"""
    a = (h3(shape), h3(ks), h3(st), h3(pd), h3(sho))
    return {
        "rulebook_conv": lambda: lib.toda_rulebook_conv(FAKE, 10, 1, *a, FAKE, 10, FAKE, FAKE, FAKE, None, None, None, 1, None),
        "gridindex_from_conv": lambda: lib.toda_gridindex_from_conv(FAKE, 10, None, 1, *a, FAKE, FAKE, FAKE, 10, None),
        "gridindex_from_bitmap": lambda: lib.toda_gridindex_from_bitmap(FAKE, 1, *a, FAKE, FAKE, FAKE, 10, 0, None),
    }


def test_strided_builders_refuse_a_kernel_volume_above_64():
    ks, st, pd = RC.REFUSED_CONV
    shape = (8, 8, 8)
    for who, call in conv_calls(L.load(), shape, ks, st, pd, RC.conv_out_shape(shape, ks, st, pd)).items():
        assert refused(call(), who, "volume"), who


def test_strided_builders_refuse_an_output_shape_off_the_formula():
    shape, ks, st, pd = (8, 9, 10), (3, 3, 3), (2, 2, 2), (1, 1, 1)
    good = RC.conv_out_shape(shape, ks, st, pd)
    for axis in range(3):
        for d in (-1, 1):
            sho = list(good)
            sho[axis] += d
            for who, call in conv_calls(L.load(), shape, ks, st, pd, sho).items():
                assert refused(call(), who, "shape_out[%d]" % axis), (who, sho)
    # an axis shorter than its kernel has no output cell, whatever a division that rounds towards zero makes of (in + 2p - k) / s + 1
    for who, call in conv_calls(L.load(), (4, 4, 1), (2, 2, 2), (2, 2, 2), (0, 0, 0), (2, 2, 1)).items():
        assert refused(call(), who), who


def test_from_bitmap_refuses_a_window_wider_than_128_bits_and_from_conv_does_not():
    lib = L.load()
    ks, st, pd = RC.TOO_WIDE
    shape = (2, 2, 64)
    calls = conv_calls(lib, shape, ks, st, pd, RC.conv_out_shape(shape, ks, st, pd))
    assert refused(calls["gridindex_from_bitmap"](), "gridindex_from_bitmap", "too wide")
    ks, st, pd = RC.STRIDED_GEOMS[6]
    assert 31 * st[2] + ks[2] == 128      # ... and the widest accepted one passes the same check (nothing to launch it on here)


def test_builders_refuse_bad_lattices_and_negative_sizes():
    lib = L.load()
    for batch, shape in ((0, (4, 4, 4)), (1, (4, 0, 4)), (2 ** 10, (2 ** 10, 2 ** 10, 2 ** 7))):
        assert refused(lib.toda_gridindex_from_coords(FAKE, 1, None, batch, h3(shape), FAKE, FAKE, None), "gridindex_from_coords")
        assert refused(lib.toda_gridindex_from_coords_unordered(FAKE, 1, None, batch, h3(shape), FAKE, FAKE, 0, None), "gridindex_from_coords_unordered")
        assert refused(lib.toda_gridindex_clear(FAKE, 1, None, batch, h3(shape), FAKE, None), "gridindex_clear")
    assert refused(lib.toda_gridindex_from_coords(FAKE, -1, None, 1, h3((4, 4, 4)), FAKE, FAKE, None), "n < 0")
    assert refused(lib.toda_gridindex_from_coords_unordered(FAKE, 5, None, 1, h3((4, 4, 4)), FAKE, None, 0, None), "rowof")
    assert refused(lib.toda_gridindex_clear(FAKE, -1, None, 1, h3((4, 4, 4)), FAKE, None), "n < 0")
    assert lib.toda_gridindex_clear(FAKE, 0, None, 1, h3((4, 4, 4)), FAKE, None) == 0
