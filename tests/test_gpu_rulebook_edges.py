"""The grid index and the rulebook builders of csrc/rulebook.hip and scan.cuh at their lattice and geometry edges.  Every table is
integer, every comparison is np.array_equal.  The reference is the C oracle, which test_rulebook_host.py holds against the plain
reference of tests/rulebook_cases.py on every case used here.

Which test reaches which branch:
  test_strided_geometry                  rb_conv_generic_kernel; the per-bit arm of gi_conv_bits_kernel ((1,1,9) s1, (1,1,4) s4, 3x3x3 s3);
                                         the stride-1 shift-OR arm with a 3- and an 8-wide kernel; bits32_at at both row ends with
                                         padding; the row carry of gi_scan_decode_kernel at W = 1, 11, 31, 33, 65; K = 64
  test_occupancy_through_every_builder   all-ones words, bit 0 / bit 31 masks, x - 1 of x = 0, n = 0, first / last cell, an empty sample,
                                         rb_subm_generic_kernel with dilation
  test_scan_carry_*                      the carry loop of scan_partials_kernel (from_coords and from_conv)
  test_lattice_above_2_31_cells          the 64-bit arms of gi_conv_bits_kernel and gi_scan_decode_kernel
  test_output_capacity_*                 the r < cap guards of gi_decode_kernel / gi_scan_decode_kernel, n_out_dev = true total
  test_rows_past_the_device_count_*      n_dev < n
  test_clear_*, test_row_marks_*         toda_gridindex_clear, gi_clean = 1, in_rows_marked 0 / 1
  test_refusals_*                        the argument errors, with nothing written
  test_plan_is_deterministic             two builds of one plan"""
import functools
import time

import numpy as np
import pytest
import torch

from oracle import oracle as O
from tests import rulebook_cases as RC

pytestmark = pytest.mark.gpu

SENT = -1234567      # fills every output before a call: what is still there afterwards was not written
BAND = 4096          # guard bytes on both sides of a grid-index buffer


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy()


def h3(v):
    from toda_amd import lib as L

    return L.hptr(L.host_i32([int(x) for x in v]))


@pytest.fixture(scope="module")
def lib():
    from toda_amd import lib as L

    return L.load()


def P(t):
    from toda_amd import lib as L

    return L.ptr(t)


def ok(rc, what):
    from toda_amd import lib as L

    L.check(rc, what)


def stream():
    from toda_amd import lib as L

    return L.stream()


class GiBuf:
    """A grid-index buffer of garbage bytes between two guard bands."""

    def __init__(self, lib, batch, shape, fill=0xA5):
        self.batch, self.shape, self.lay = int(batch), [int(v) for v in shape], RC.Layout(batch, shape)
        assert lib.toda_gridindex_bytes(self.batch, h3(self.shape)) == self.lay.bytes
        self.full = torch.full((self.lay.bytes + 2 * BAND,), 0x5C, dtype=torch.uint8, device="cuda")
        self.t = self.full[BAND:BAND + self.lay.bytes]
        self.t.fill_(fill)

    def intact(self):
        return bool((self.full[:BAND] == 0x5C).all()) and bool((self.full[BAND + self.lay.bytes:] == 0x5C).all())

    def cells(self):
        """[cells, 2] uint32 {bits, first rank}"""
        return host(self.t[:self.lay.cells * 8]).view(np.uint32).reshape(-1, 2)

    def row_bytes(self):
        return host(self.t[self.lay.o_rows:self.lay.o_rows + self.lay.rows])


def cells_of(gi):
    """the {bits, first rank} words of an ops.GridIndex"""
    lay = RC.Layout(gi.batch, gi.shape)
    return host(gi.buf[:lay.cells * 8]).view(np.uint32).reshape(-1, 2)


def assert_canonical_index(gi, coords):
    """the whole cell region of a canonically ranked index: occupancy words and the exclusive prefix of their popcounts"""
    assert np.array_equal(cells_of(gi), RC.canonical_cells(coords, gi.batch, gi.shape))


def assert_unordered_index(cells, row_bytes, rowof, idx, batch, shape):
    """toda_gridindex_from_coords_unordered hands ranks out per occupied word, in no fixed order: the bits and the row bytes are
    exact, the ranks are a permutation of [0, n) that keeps the sites of one word together in ascending order, and rowof undoes it"""
    n = len(idx)
    assert np.array_equal(cells[:, 0], RC.bitmap_words(idx, batch, shape))
    assert np.array_equal(row_bytes, RC.row_bytes(idx, batch, shape))
    assert not cells[cells[:, 0] == 0, 1].any()
    r = RC.ranks(cells, RC.lin_keys(idx, shape))
    assert np.array_equal(np.sort(r), np.arange(n))
    assert np.array_equal(rowof[r], np.arange(n))


@functools.lru_cache(maxsize=None)
def conv_ref(name, order, geom):
    """oracle tables of a named coordinate set (computed once): order 0 = canonical rows, 1 = shuffled"""
    batch, shape, sites = named_sites(name)
    return O.rulebook_conv(sites[order], batch, list(shape), *geom)


@functools.lru_cache(maxsize=None)
def named_sites(name):
    if name.startswith("lattice-"):
        l = int(name.split("-")[1])
        shape, batch = RC.LATTICES[l]
        return batch, shape, RC.strided_sites(l)
    if name == "carry":
        return RC.CARRY_BATCH, RC.CARRY_SHAPE, RC.carry_sites()
    if name == "big":
        return RC.BIG_BATCH, RC.BIG_SHAPE, RC.big_sites()
    return RC.occupancy_sets()[name]


def assert_conv_equal(ref, out_indices, out_shape, rb):
    io0, sho0, o2i0, i2o0, cnt0 = ref
    assert [int(v) for v in out_shape] == sho0
    assert np.array_equal(host(out_indices), io0)
    assert np.array_equal(host(rb.nbr_fwd), o2i0)
    assert np.array_equal(host(rb.nbr_bwd), i2o0)
    assert np.array_equal(host(rb.pair_cnt), cnt0)


def lazy_conv(name, geom, order=0):
    """ops.build_conv_rulebook (toda_gridindex_from_conv: atomics, three-kernel scan, gi_decode_kernel)"""
    from toda_amd import ops

    batch, shape, sites = named_sites(name)
    io1, sho1, rb, gi = ops.build_conv_rulebook(dev(sites[order]), batch, list(shape), *geom)
    ref = conv_ref(name, order, geom)
    assert_conv_equal(ref, io1, sho1, rb)
    assert_canonical_index(gi, ref[0])
    return io1, sho1, gi


def plan_conv(name, geom, order=1):
    """a one-step ops.build_index_plan (toda_gridindex_from_coords_unordered, then toda_gridindex_from_bitmap)"""
    from toda_amd import ops

    batch, shape, sites = named_sites(name)
    steps = [{"kind": "conv", "key": "c", "ksize": list(geom[0]), "stride": list(geom[1]), "padding": list(geom[2])}]
    e = ops.build_index_plan(dev(sites[order]), batch, list(shape), steps, training=False)["c"]
    ref = conv_ref(name, order, geom)
    assert_conv_equal(ref, e["out_indices"], e["out_shape"], e["rb"])
    return e


# ================================================================================================ strided geometries
@pytest.mark.parametrize("g,l", RC.STRIDED_CASES, ids=[RC.geom_id(g) + "-" + RC.lattice_id(l) for g, l in RC.STRIDED_CASES])
def test_strided_geometry(g, l):
    """Both builders on every geometry x lattice, except RC.EMPTY_OUTPUT: the combinations whose output lattice has no cell
    (an axis smaller than its kernel minus the padding), which test_rulebook_host.py proves to be exactly those."""
    geom = RC.STRIDED_GEOMS[g]
    lazy_conv("lattice-%d" % l, geom, order=0)
    e = plan_conv("lattice-%d" % l, geom, order=1)
    assert_canonical_index(e["gi"], conv_ref("lattice-%d" % l, 1, geom)[0])


# ================================================================================================ occupancy
@pytest.mark.parametrize("name", RC.OCCUPANCY_NAMES)
def test_occupancy_through_every_builder(name):
    from toda_amd import ops

    batch, shape, (canon, shuf) = named_sites(name)
    shape = list(shape)
    # canonical ranks (scan) on the shuffled list: rowof is the sort
    gi = ops.GridIndex.from_coords(dev(shuf), batch, shape)
    assert_canonical_index(gi, shuf)
    if len(shuf):
        assert np.array_equal(host(gi.rowof)[:len(shuf)], np.argsort(RC.lin_keys(shuf, shape), kind="stable"))
    for ks, dil in RC.SUBM_KERNELS:
        nbr0, cnt0 = O.rulebook_subm(shuf, batch, shape, ks, dil)
        rb, _ = ops.build_subm_rulebook(dev(shuf), batch, shape, ks, dil, grid_index=gi)
        assert np.array_equal(host(rb.nbr_fwd), nbr0) and np.array_equal(host(rb.pair_cnt), cnt0)
        # ... and on an index of its own (toda_gridindex_from_coords_unordered)
        rb, _ = ops.build_subm_rulebook(dev(shuf), batch, shape, ks, dil)
        assert np.array_equal(host(rb.nbr_fwd), nbr0) and np.array_equal(host(rb.pair_cnt), cnt0)
    io1, sho1, gi_out = lazy_conv(name, RC.OCC_CONV, order=0)
    plan_conv(name, RC.OCC_CONV, order=1)
    # the output set's index serves the next SubM layer with rowof = None
    nbr0, cnt0 = O.rulebook_subm(host(io1), batch, sho1)
    rb, _ = ops.build_subm_rulebook(io1, batch, sho1, 3, 1, grid_index=gi_out)
    assert np.array_equal(host(rb.nbr_fwd), nbr0) and np.array_equal(host(rb.pair_cnt), cnt0)


# ================================================================================================ scan carry
def test_scan_carry_from_coords_and_subm():
    from toda_amd import ops

    batch, shape, (canon, shuf) = named_sites("carry")
    gi = ops.GridIndex.from_coords(dev(shuf), batch, list(shape))
    assert_canonical_index(gi, shuf)
    assert np.array_equal(host(gi.rowof), np.argsort(RC.lin_keys(shuf, shape), kind="stable"))
    nbr0, cnt0 = O.rulebook_subm(shuf, batch, list(shape))
    rb, _ = ops.build_subm_rulebook(dev(shuf), batch, list(shape), 3, 1, grid_index=gi)
    assert np.array_equal(host(rb.nbr_fwd), nbr0) and np.array_equal(host(rb.pair_cnt), cnt0)


def test_scan_carry_from_conv():
    lazy_conv("carry", RC.CARRY_CONV, order=1)


# ================================================================================================ 64-bit arithmetic
def test_lattice_above_2_31_cells():
    """[9, 15450, 15450]: input and output lattice of a 3x3x3 stride-1 plan step both hold just over 2^31 cells (2^26 words), the
    smallest shape at which gi_conv_bits_kernel and gi_scan_decode_kernel leave their 32-bit arithmetic.  0.54 GB per index."""
    from toda_amd import ops

    batch, shape, (canon, shuf) = named_sites("big")
    ref = conv_ref("big", 1, RC.BIG_CONV)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e = plan_conv("big", RC.BIG_CONV, order=1)
    torch.cuda.synchronize()
    print("2^31-cell plan step: %.3f s for %d -> %d sites" % (time.perf_counter() - t0, len(shuf), len(ref[0])))
    # the output index, on the device: the occupied words, their bits and their ranks
    lay = RC.Layout(batch, shape)
    words = e["gi"].buf[:lay.cells * 8].view(torch.int32).view(-1, 2)
    at = torch.nonzero(words[:, 0]).flatten()
    keys = RC.lin_keys(ref[0], shape)
    want_at, first = np.unique(keys >> 5, return_index=True)
    assert np.array_equal(host(at), want_at)
    got = host(words[at]).view(np.uint32)
    want_bits = np.zeros(len(want_at), np.uint32)
    np.bitwise_or.at(want_bits, np.searchsorted(want_at, keys >> 5), np.uint32(1) << (keys & 31).astype(np.uint32))
    assert np.array_equal(got[:, 0], want_bits) and np.array_equal(got[:, 1], first.astype(np.uint32))
    del words, at, e
    torch.cuda.empty_cache()


# ================================================================================================ capacity
def guarded_rows(cap):
    """int32 [cap, 4] between two bands of SENT"""
    full = torch.full(((cap + 128) * 4,), SENT, dtype=torch.int32, device="cuda")
    return full, full[256:256 + cap * 4]


def check_capped(full, cap, want, n_out_dev):
    full = host(full)
    assert int(host(n_out_dev)[0]) == len(want)
    assert np.array_equal(full[256:256 + cap * 4].reshape(-1, 4), want[:cap])
    assert (full[:256] == SENT).all() and (full[256 + cap * 4:] == SENT).all(), "rows at or past out_cap were written"


@pytest.mark.parametrize("name,g", [("lattice-1", 1), ("lattice-0", 0), ("lattice-1", 7), ("full-3x4x33x2", 3)])
def test_output_capacity_is_respected_and_the_true_count_reported(lib, name, g):
    geom = RC.STRIDED_GEOMS[g]
    batch, shape, (canon, shuf) = named_sites(name)
    want = conv_ref(name, 1, geom)[0]
    sho = RC.conv_out_shape(shape, *geom)
    a = (h3(shape), h3(geom[0]), h3(geom[1]), h3(geom[2]), h3(sho))
    idx = dev(shuf)
    gi_in = GiBuf(lib, batch, shape)
    rowof = torch.empty((len(shuf),), dtype=torch.int32, device="cuda")
    ok(lib.toda_gridindex_from_coords_unordered(P(idx), len(shuf), None, batch, h3(shape), P(gi_in.t), P(rowof), 0, stream()), "unordered")
    assert len(want) > 8
    for cap in (len(want) // 2, 1, 0, len(want)):
        for builder in ("from_conv", "from_bitmap"):
            gi_out = GiBuf(lib, batch, sho)
            full, rows = guarded_rows(cap)
            n_out = torch.full((1,), SENT, dtype=torch.int32, device="cuda")
            if builder == "from_conv":
                ok(lib.toda_gridindex_from_conv(P(idx), len(shuf), None, batch, *a, P(gi_out.t), P(full) + 1024, P(n_out), cap, stream()), builder)
            else:
                ok(lib.toda_gridindex_from_bitmap(P(gi_in.t), batch, *a, P(gi_out.t), P(full) + 1024, P(n_out), cap, 1, stream()), builder)
            check_capped(full, cap, want, n_out)
            # the index itself is complete whatever the capacity
            assert np.array_equal(gi_out.cells(), RC.canonical_cells(want, batch, sho)) and gi_out.intact()
    assert gi_in.intact()


# ================================================================================================ n_dev < n
def test_rows_past_the_device_count_are_ignored(lib):
    (shape, batch) = RC.LATTICES[1]
    canon, shuf = RC.clustered(batch, shape, seed=55, n_per_batch=1200)
    n_dev = len(shuf) - 300
    assert n_dev > 1024                      # more than one block of the rank allocator
    valid, rest = shuf[:n_dev], shuf[n_dev:]
    rng = np.random.default_rng(5)
    garbage = np.concatenate([rest, np.stack([rng.integers(0, batch, 400), rng.integers(0, shape[0], 400), rng.integers(0, shape[1], 400),
                                               rng.integers(0, shape[2], 400)], 1).astype(np.int32)])
    everything = np.ascontiguousarray(np.concatenate([valid, garbage]))
    n = len(everything)
    idx, count = dev(everything), dev(np.array([n_dev], np.int32))
    gi = GiBuf(lib, batch, shape)
    rowof = torch.full((n,), SENT, dtype=torch.int32, device="cuda")
    ok(lib.toda_gridindex_from_coords_unordered(P(idx), n, P(count), batch, h3(shape), P(gi.t), P(rowof), 0, stream()), "unordered")
    r = host(rowof)
    assert_unordered_index(gi.cells(), gi.row_bytes(), r[:n_dev], valid, batch, shape)
    assert (r[n_dev:] == SENT).all() and gi.intact()
    # the truncated list on its own gives the same bits and row bytes
    gi2 = GiBuf(lib, batch, shape)
    rowof2 = torch.full((n_dev,), SENT, dtype=torch.int32, device="cuda")
    ok(lib.toda_gridindex_from_coords_unordered(P(idx), n_dev, None, batch, h3(shape), P(gi2.t), P(rowof2), 0, stream()), "unordered")
    assert np.array_equal(gi2.cells()[:, 0], gi.cells()[:, 0]) and np.array_equal(gi2.row_bytes(), gi.row_bytes())
    assert_unordered_index(gi2.cells(), gi2.row_bytes(), host(rowof2), valid, batch, shape)
    # the SubM table of the valid rows
    nbr0, cnt0 = O.rulebook_subm(valid, batch, list(shape))
    for g_, ro in ((gi, rowof), (gi2, rowof2)):
        nbr = torch.full((27, n_dev), SENT, dtype=torch.int32, device="cuda")
        cnt = torch.full((27,), SENT, dtype=torch.int32, device="cuda")
        ok(lib.toda_rulebook_subm(P(idx), n_dev, batch, h3(shape), h3((3, 3, 3)), h3((1, 1, 1)), P(g_.t), P(ro), P(nbr), P(cnt), 0, stream()), "subm")
        assert np.array_equal(host(nbr), nbr0) and np.array_equal(host(cnt), cnt0)
    # the same through toda_gridindex_from_coords (canonical ranks)
    gi3 = GiBuf(lib, batch, shape)
    rowof3 = torch.full((n,), SENT, dtype=torch.int32, device="cuda")
    ok(lib.toda_gridindex_from_coords(P(idx), n, P(count), batch, h3(shape), P(gi3.t), P(rowof3), stream()), "from_coords")
    assert np.array_equal(gi3.cells(), RC.canonical_cells(valid, batch, shape)) and gi3.intact()
    r3 = host(rowof3)
    assert np.array_equal(r3[:n_dev], np.argsort(RC.lin_keys(valid, shape), kind="stable")) and (r3[n_dev:] == SENT).all()


# ================================================================================================ clear and reuse
OUTSIDE = np.array([[-1, 0, 0, 0], [9, 1, 1, 1], [0, -1, 2, 2], [0, 7, 3, 3], [1, 2, 33, 4], [1, 2, -5, 4], [0, 3, 4, 65], [0, 3, 4, -1],
                    [2 ** 30, 2 ** 30, 2 ** 30, 2 ** 30], [-2 ** 31, -2 ** 31, -2 ** 31, -2 ** 31]], np.int32)


def test_clear_restores_zeros_and_a_clean_rebuild_equals_a_fresh_one(lib):
    (shape, batch) = RC.LATTICES[1]
    lay = RC.Layout(batch, shape)
    _, set_a = RC.strided_sites(1)
    _, set_b = RC.clustered(batch, shape, seed=77)
    assert not np.array_equal(RC.bitmap_words(set_a, batch, shape), RC.bitmap_words(set_b, batch, shape))
    gi = GiBuf(lib, batch, shape)
    a_dev = dev(np.ascontiguousarray(np.insert(set_a, [0, 3, 3, 500, 500, 900, 1000, 1100, len(set_a), len(set_a)], OUTSIDE, axis=0)))
    rowof = torch.empty((len(a_dev),), dtype=torch.int32, device="cuda")
    ok(lib.toda_gridindex_from_coords_unordered(P(a_dev), len(a_dev), None, batch, h3(shape), P(gi.t), P(rowof), 0, stream()), "unordered")
    assert np.array_equal(gi.cells()[:, 0], RC.bitmap_words(set_a, batch, shape)) and np.array_equal(gi.row_bytes(), RC.row_bytes(set_a, batch, shape))
    ok(lib.toda_gridindex_clear(P(a_dev), len(a_dev), None, batch, h3(shape), P(gi.t), stream()), "clear")
    zeros = torch.zeros_like(gi.t)
    assert torch.equal(gi.t[:lay.cells * 8], zeros[:lay.cells * 8]), "the cell words are not all zero again"
    assert torch.equal(gi.t[lay.o_rows:lay.o_rows + lay.rows], zeros[:lay.rows]), "the row bytes are not all zero again"
    assert gi.intact()
    # set B on the cleaned buffer (gi_clean = 1) and on a fresh one (gi_clean = 0)
    fresh = GiBuf(lib, batch, shape, fill=0x3C)
    b_dev = dev(set_b)
    out = {}
    geom = RC.STRIDED_GEOMS[3]
    sho = RC.conv_out_shape(shape, *geom)
    a = (h3(shape), h3(geom[0]), h3(geom[1]), h3(geom[2]), h3(sho))
    want = O.rulebook_conv(set_b, batch, list(shape), *geom)[0]
    nbr0, cnt0 = O.rulebook_subm(set_b, batch, list(shape))
    for tag, buf, clean in (("reused", gi, 1), ("fresh", fresh, 0)):
        ro = torch.full((len(set_b),), SENT, dtype=torch.int32, device="cuda")
        ok(lib.toda_gridindex_from_coords_unordered(P(b_dev), len(set_b), None, batch, h3(shape), P(buf.t), P(ro), clean, stream()), "unordered")
        assert_unordered_index(buf.cells(), buf.row_bytes(), host(ro), set_b, batch, shape)
        nbr = torch.full((27, len(set_b)), SENT, dtype=torch.int32, device="cuda")
        cnt = torch.full((27,), SENT, dtype=torch.int32, device="cuda")
        ok(lib.toda_rulebook_subm(P(b_dev), len(set_b), batch, h3(shape), h3((3, 3, 3)), h3((1, 1, 1)), P(buf.t), P(ro), P(nbr), P(cnt), 0, stream()), "subm")
        assert np.array_equal(host(nbr), nbr0) and np.array_equal(host(cnt), cnt0)
        for marked in (0, 1):
            gi_out = GiBuf(lib, batch, sho, fill=0x11 * (marked + 1))
            rows = torch.full((len(want), 4), SENT, dtype=torch.int32, device="cuda")
            n_out = torch.full((1,), SENT, dtype=torch.int32, device="cuda")
            ok(lib.toda_gridindex_from_bitmap(P(buf.t), batch, *a, P(gi_out.t), P(rows), P(n_out), len(want), marked, stream()), "from_bitmap")
            assert int(host(n_out)[0]) == len(want) and gi_out.intact()
            out[tag, marked] = (host(rows).tobytes(), gi_out.cells().tobytes())
        assert buf.intact()
    assert np.array_equal(gi.cells()[:, 0], fresh.cells()[:, 0]) and np.array_equal(gi.row_bytes(), fresh.row_bytes())
    assert out["reused", 0] == out["reused", 1] == out["fresh", 0] == out["fresh", 1]
    assert out["fresh", 0] == (want.tobytes(), RC.canonical_cells(want, batch, sho).astype(np.uint32).tobytes())


@pytest.mark.parametrize("name", ["lattice-1", "sample-1-of-3-empty"])
def test_row_marks_do_not_change_the_output_set_on_sparse_rows(lib, name):
    """sets that leave whole input rows (b, z, y) without a site, so in_rows_marked = 1 really skips some"""
    batch, shape, (canon, shuf) = named_sites(name)
    gi = GiBuf(lib, batch, shape)
    idx = dev(shuf)
    rowof = torch.empty((len(shuf),), dtype=torch.int32, device="cuda")
    ok(lib.toda_gridindex_from_coords_unordered(P(idx), len(shuf), None, batch, h3(shape), P(gi.t), P(rowof), 0, stream()), "unordered")
    assert 0 < int(gi.row_bytes().sum()) < len(gi.row_bytes())
    for geom in (RC.STRIDED_GEOMS[7], RC.STRIDED_GEOMS[5], RC.STRIDED_GEOMS[6], RC.OCC_CONV):
        sho = RC.conv_out_shape(shape, *geom)
        want = O.rulebook_conv(shuf, batch, list(shape), *geom)[0]
        got = []
        for marked in (0, 1):
            gi_out = GiBuf(lib, batch, sho)
            rows = torch.full((len(want), 4), SENT, dtype=torch.int32, device="cuda")
            n_out = torch.full((1,), SENT, dtype=torch.int32, device="cuda")
            ok(lib.toda_gridindex_from_bitmap(P(gi.t), batch, h3(shape), h3(geom[0]), h3(geom[1]), h3(geom[2]), h3(sho), P(gi_out.t), P(rows),
                                              P(n_out), len(want), marked, stream()), "from_bitmap")
            assert int(host(n_out)[0]) == len(want) and gi_out.intact()
            got.append((host(rows).tobytes(), gi_out.cells().tobytes()))
        assert got[0] == got[1] == (want.tobytes(), RC.canonical_cells(want, batch, sho).astype(np.uint32).tobytes())


# ================================================================================================ refusals
def test_refusals_return_the_argument_error_and_write_nothing(lib):
    from toda_amd import ops

    (shape, batch) = RC.LATTICES[0]
    canon, shuf = RC.strided_sites(0)
    n = len(shuf)
    idx = dev(shuf)
    gi = ops.GridIndex.from_coords(idx, batch, list(shape))
    before = gi.buf.clone()
    out = torch.full((75 * max(n, 4 * 1500),), SENT, dtype=torch.int32, device="cuda")
    cnt = torch.full((128,), SENT, dtype=torch.int32, device="cuda")

    def untouched():
        torch.cuda.synchronize()
        return bool((out == SENT).all()) and bool((cnt == SENT).all()) and torch.equal(gi.buf, before)

    for ks, word in RC.REFUSED_SUBM:
        with pytest.raises(RuntimeError, match=r"code -1.*rulebook_subm.*" + word):
            ok(lib.toda_rulebook_subm(P(idx), n, batch, h3(shape), h3(ks), h3((1, 1, 1)), P(gi.buf), P(gi.rowof), P(out), P(cnt), 0, stream()), "subm")
        with pytest.raises(RuntimeError, match="code -1"):
            ops.build_subm_rulebook(idx, batch, list(shape), ks, 1, grid_index=gi)
        assert untouched()
    ks, st, pd = RC.REFUSED_CONV
    sho = RC.conv_out_shape(shape, ks, st, pd)
    a = (h3(shape), h3(ks), h3(st), h3(pd), h3(sho))
    with pytest.raises(RuntimeError, match="code -1.*volume"):
        ok(lib.toda_rulebook_conv(P(idx), n, batch, *a, P(gi.buf), n, P(out), P(out), P(cnt), None, None, None, 0, stream()), "conv")
    with pytest.raises(RuntimeError, match="code -1.*volume"):
        ok(lib.toda_gridindex_from_conv(P(idx), n, None, batch, *a, P(gi.buf), P(out), P(cnt), 1500, stream()), "from_conv")
    with pytest.raises(RuntimeError, match="code -1.*volume"):
        ops.build_conv_rulebook(idx, batch, list(shape), ks, st, pd)
    assert untouched()
    ks, st, pd = RC.TOO_WIDE
    sho = RC.conv_out_shape(shape, ks, st, pd)
    a = (h3(shape), h3(ks), h3(st), h3(pd), h3(sho))
    with pytest.raises(RuntimeError, match="code -1.*too wide"):
        ok(lib.toda_gridindex_from_bitmap(P(gi.buf), batch, *a, P(out), P(out), P(cnt), 1500, 0, stream()), "from_bitmap")
    with pytest.raises(RuntimeError, match="code -1.*too wide"):
        ops.build_index_plan(idx, batch, list(shape), [{"kind": "conv", "key": "c", "ksize": list(ks), "stride": list(st), "padding": list(pd)}],
                             training=False)
    assert untouched()
    # a shape_out off the formula, on every entry point that takes one
    ks, st, pd = RC.STRIDED_GEOMS[3]
    sho = RC.conv_out_shape(shape, ks, st, pd)
    for axis in range(3):
        bad = list(sho)
        bad[axis] += 1
        a = (h3(shape), h3(ks), h3(st), h3(pd), h3(bad))
        with pytest.raises(RuntimeError, match=r"code -1.*shape_out\[%d\]" % axis):
            ok(lib.toda_gridindex_from_conv(P(idx), n, None, batch, *a, P(gi.buf), P(out), P(cnt), 1500, stream()), "from_conv")
        with pytest.raises(RuntimeError, match=r"code -1.*shape_out\[%d\]" % axis):
            ok(lib.toda_gridindex_from_bitmap(P(gi.buf), batch, *a, P(out), P(out), P(cnt), 1500, 0, stream()), "from_bitmap")
        with pytest.raises(RuntimeError, match=r"code -1.*shape_out\[%d\]" % axis):
            ok(lib.toda_rulebook_conv(P(idx), n, batch, *a, P(gi.buf), n, P(out), P(out), P(cnt), None, None, None, 0, stream()), "conv")
    assert untouched()


def test_lazy_builder_takes_the_window_that_from_bitmap_refuses():
    lazy_conv("lattice-1", RC.TOO_WIDE, order=1)
    lazy_conv("lattice-5", RC.TOO_WIDE, order=0)


# ================================================================================================ determinism
def test_plan_is_deterministic():
    from toda_amd import ops

    (shape, batch) = RC.LATTICES[1]
    _, shuf = RC.strided_sites(1)
    steps = [
        {"kind": "subm", "key": "subm1", "ksize": [3, 3, 3], "dilation": [1, 1, 1]},
        {"kind": "conv", "key": "down1", "ksize": [3, 3, 3], "stride": [2, 2, 2], "padding": [1, 1, 1]},
        {"kind": "subm", "key": "subm2", "ksize": [3, 3, 5], "dilation": [1, 1, 1]},
        {"kind": "conv", "key": "down2", "ksize": [1, 3, 3], "stride": [1, 2, 2], "padding": [0, 1, 1]},
        {"kind": "subm", "key": "subm3", "ksize": [3, 3, 3], "dilation": [1, 1, 1]},
    ]

    def tables():
        plan = ops.build_index_plan(dev(shuf), batch, list(shape), steps, training=False)
        out = {}
        for key, e in plan.items():
            out[key] = [host(e["rb"].nbr_fwd), host(e["rb"].nbr_bwd), host(e["rb"].pair_cnt)]
            if e["kind"] == "conv":
                out[key] += [host(e["out_indices"]), np.asarray(e["out_shape"]), cells_of(e["gi"])]
        return out

    first, second = tables(), tables()
    assert sorted(first) == sorted(second) == sorted(s["key"] for s in steps)
    for key in first:
        assert len(first[key]) == len(second[key])
        for a, b in zip(first[key], second[key]):
            assert np.array_equal(a, b), key
    # ... and they are the right ones
    cur, cur_shape = shuf, list(shape)
    for s in steps:
        if s["kind"] == "subm":
            nbr0, cnt0 = O.rulebook_subm(cur, batch, cur_shape, s["ksize"], s["dilation"])
            assert np.array_equal(first[s["key"]][0], nbr0) and np.array_equal(first[s["key"]][2], cnt0)
        else:
            io0, sho0, o2i0, i2o0, cnt0 = O.rulebook_conv(cur, batch, cur_shape, s["ksize"], s["stride"], s["padding"])
            got = first[s["key"]]
            assert np.array_equal(got[0], o2i0) and np.array_equal(got[1], i2o0) and np.array_equal(got[2], cnt0) and np.array_equal(got[3], io0)
            cur, cur_shape = io0, sho0
