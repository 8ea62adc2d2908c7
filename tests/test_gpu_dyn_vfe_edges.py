"""The dynamic voxel index (csrc/dynvox.hip over radix_sort.cuh and scan.cuh) and its segment kernels on the MI355X at the edges
the workload-sized clouds of test_gpu_dyn_vfe.py never reach: points on cell boundaries and their fp32 neighbours, every pass count
of the radix sort and partial waves / rounds / tiles of its scatter, scans with a second sweep of partials, merge keys above 2^31,
bitmap word edges, the batch column, row widths, and the segment kernels through the C ABI on hand-built CSR tables with poisoned
outputs.  The index is bit-exact against torch_dyn_index (check_index) and against the hand-written index of the case; sums are
bit-equal to the documented order restated in numpy float32 (tests/dyn_vfe_cases.py).  The hard voxeliser shares the cell expression
and runs on the same lattice."""
import numpy as np
import pytest
import torch

from tests import dyn_vfe_cases as D
from tests.test_gpu_dyn_vfe import check_index
from tests.test_gpu_input_plan import oracle_batch
from toda_amd import ops

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
ARRAYS = ("keep", "rows", "inv", "cnt", "coords", "seg_off", "seg_pts")


def poison(shape, dtype=torch.float32, value=float("nan")):
    """Leave a block of this size filled with `value` in torch's caching allocator: the next output of that size usually lands in
    it, so an element a kernel never writes reads as NaN (or -1) instead of an earlier, correct result."""
    torch.full(shape, value, dtype=dtype, device=DEV)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits(a):
    """float32 as its bit pattern: -0.0 and +0.0 differ"""
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def check_twice(pts, g):
    """check_index (bit-exact against torch_dyn_index, every segment its voxel's rows ascending), then a second call: same bits"""
    idx = check_index(pts, g.pc_range, g.voxel_size, g.batch, g.pillar)
    again = ops.dyn_voxel_index(torch.from_numpy(pts).to(DEV), g.pc_range, g.voxel_size, g.batch, g.pillar)
    for a in ARRAYS:
        assert torch.equal(getattr(idx, a), getattr(again, a)), a
    return idx


def check_case(case):
    """... and against the index the case wrote down by hand"""
    idx = check_twice(case.pts, case.geom)
    assert idx.M == case.M and idx.K == case.K
    assert np.array_equal(idx.keep.cpu().numpy(), case.keep) and np.array_equal(idx.inv.cpu().numpy(), case.inv)
    assert np.array_equal(idx.cnt.cpu().numpy(), case.cnt) and np.array_equal(idx.coords.cpu().numpy(), case.coords)
    return idx


# ---------------------------------------------------------------------------------------------- the index
@pytest.mark.parametrize("pillar", [True, False])
@pytest.mark.parametrize("name", sorted(D.LATTICE_GEOMETRIES))
def test_index_on_the_boundary_lattice(name, pillar):
    """every cell boundary of every tested axis, one ulp below and one above: dv_key's fp32 floor((p - lo) / size) bit for bit"""
    pc_range, vs = D.LATTICE_GEOMETRIES[name]
    pts = D.boundary_lattice(pc_range, vs, pillar, 2, extra_x=D.DENORMAL_X if name == "lo_zero" else ())
    idx = check_twice(pts, D.Geom(pc_range, vs, pillar, 2))
    assert 0 < idx.K < len(pts)


@pytest.mark.parametrize("m,rag", D.SORT_M_CASES)
def test_index_at_the_sort_pass_thresholds(m, rag):
    """M = 1 .. 256: one pass (the result is in the second buffer pair), .. 65536: two, 65537: three"""
    check_case(D.sort_m_case(m, rag))


@pytest.mark.parametrize("k,m", D.SORT_K_CASES)
def test_index_at_the_scatter_wave_round_and_tile_edges(k, m):
    check_case(D.sort_k_case(k, m))


@pytest.mark.parametrize("n", D.SCAN_N)
def test_index_at_the_scan_tile_and_partial_sweep_edges(n):
    check_case(D.scan_case(n))


@pytest.mark.parametrize("pillar", [False, True])
def test_index_with_merge_keys_above_int32(pillar):
    """24 Waymo samples: the voxel key space passes 2^31 (sample 23, x cell >= 1105); the pillar one does not and is the control"""
    case = D.wide_case(pillar)
    idx = check_case(case)
    assert int(idx.coords[-1, 0]) == 23 and (case.keys.max() > 2 ** 31) == (not pillar)


@pytest.mark.parametrize("name", sorted(D.WORD_VARIANTS))
def test_index_at_the_bitmap_word_edges(name):
    check_case(D.word_case(name))


def test_index_batch_column_follows_torch_dyn_index():
    """0 <= v < batch is kept and truncated (0.5 -> 0, batch - 0.5 -> batch - 1, -0.0 -> 0); batch, -0.5, NaN and 1e9 are dropped.  The
    kernel and torch_dyn_index agree: both read points[:, 0] as the reference does and drop what is no sample of the batch."""
    g, pts = D.batch_column_case(3)
    idx = check_twice(pts, g)
    assert idx.K == 5 * 36 and sorted(set(idx.coords[:, 0].tolist())) == [0, 2]


@pytest.mark.parametrize("width", D.WIDTHS)
def test_index_row_widths(width):
    check_case(D.width_case(width))


@pytest.mark.parametrize("pillar", [True, False])
def test_index_without_rows_and_with_one(pillar):
    g = D.Geom(*D.WAYMO_VOXEL, pillar, 2)
    idx = check_twice(np.zeros((0, 6), np.float32), g)
    assert idx.M == 0 and idx.K == 0 and idx.seg_off.cpu().tolist() == [0]
    one = D.cell_centres(g, [[1, 1503, 0, 39]], [1], seed=0, n_drop=0)
    idx = check_case(one)
    assert idx.K == 1 and idx.seg_pts.cpu().tolist() == [0] and idx.seg_off.cpu().tolist() == [0, 1]
    check_case(D.cell_centres(g, [[1, 1503, 0, 39]], [1], seed=0))      # ... and among dropped rows


# ---------------------------------------------------------------------------------------------- the hard voxeliser on the lattice
@pytest.mark.parametrize("name", ["waymo_voxel", "kitti_lo_zero"])
def test_voxelize_bit_exact_on_the_boundary_lattice(name):
    """voxelize.hip's vox_cell is the same fp32 expression: coords, counts and voxels against the sequential voxeliser, bit for bit"""
    from oracle import oracle as O

    rng, vs = D.WAYMO_VOXEL if name == "waymo_voxel" else D.KITTI_HARD
    pts = np.ascontiguousarray(D.boundary_lattice(rng, vs, False, 1, extra_x=() if name == "waymo_voxel" else D.DENORMAL_X)[:, 1:])
    P, cap = 5, len(pts)
    v0, c0, n0 = O.voxelize_hard(pts, rng, vs, P, cap)
    assert 0 < n0.sum() < len(pts)
    v1, c1, n1 = ops.voxelize(dev(pts), rng, vs, P, cap)
    assert np.array_equal(c1.cpu().numpy(), c0) and np.array_equal(n1.cpu().numpy(), n0) and np.array_equal(bits(v1.cpu().numpy()), bits(v0))
    clouds = [pts, np.ascontiguousarray(pts[::-1]), pts[: len(pts) // 2]]
    v0, c0, n0 = oracle_batch(clouds, rng, vs, P, cap)
    v1, c1, n1 = ops.voxelize_batch([dev(p) for p in clouds], rng, vs, P, cap)
    assert np.array_equal(c1.cpu().numpy(), c0) and np.array_equal(n1.cpu().numpy(), n0) and np.array_equal(bits(v1.cpu().numpy()), bits(v0))


# ---------------------------------------------------------------------------------------------- segment kernels
def table_index(seg_off, seg_pts, inv, rows=None):
    """a DynVoxelIndex over a hand-built CSR table (what the segment kernels read of it)"""
    return ops.DynVoxelIndex(None, None if rows is None else dev(rows), dev(inv), dev(np.diff(seg_off).astype(np.int32)),
                             torch.zeros((len(seg_off) - 1, 4), dtype=torch.int32, device=DEV), dev(seg_off), dev(seg_pts), True)


def hot_cloud_index(width=6, seed=0):
    pts = D.decorate_cloud(*D.WAYMO_PILLAR, width, seed)
    t = dev(pts)
    idx = ops.dyn_voxel_index(t, *D.WAYMO_PILLAR, 2, True)
    assert int(idx.cnt.max()) >= 4097 and int((idx.cnt == 1).sum()) > 100
    return pts, t, idx


@pytest.mark.parametrize("ncol", [1, 3, 5, 33])
def test_seg_sum_is_the_documented_fp32_order(ncol):
    """ncol < ld at col0 = 0, 1 and ld - ncol, with and without a rowmap, sum and mean, M * ncol around a block of 256 threads, segments
    of 1 .. 4097 rows: bit-equal to the running fp32 sum (and one fp32 division), and inside the recursive-summation bound of fp64.
    (A column's sum does not depend on its neighbours: the references run once over all ld columns and are sliced.)"""
    rng = np.random.default_rng(ncol)
    ld = ncol + 2
    for m in D.grid_tail_ms(ncol):
        seg_off, seg_pts, inv = D.csr_table(D.mixed_lengths(m, rot=m), seed=m)
        k = int(seg_off[-1])
        src = (rng.standard_normal((k + 40, ld)) * 10 + 3).astype(np.float32)
        index, src_dev = table_index(seg_off, seg_pts, inv), dev(src)
        for rm in (None, rng.permutation(k + 40)[:k].astype(np.int32)):
            want = D.seq_sum_f32(src, seg_off, seg_pts, rm, 0, ld, False)
            ref = D.seq_sum_f64(src, seg_off, seg_pts, rm, 0, ld, False)
            mag = D.seq_sum_f64(np.abs(src), seg_off, seg_pts, rm, 0, ld, False)
            for col0 in (0, 1, ld - ncol):
                for divide in (False, True):
                    cols = slice(col0, col0 + ncol)
                    w, r = (D.seg_mean(a[:, cols], seg_off) if divide else a[:, cols] for a in (want, ref))
                    poison((m, ncol))
                    got = ops.dyn_seg_sum(src_dev, index, col0, ncol, rowmap=None if rm is None else dev(rm), mean=divide).cpu().numpy()
                    bound = D.seq_sum_bound(src, seg_off, seg_pts, rm, col0, ncol, divide, r, mag=mag[:, cols])
                    assert np.all(np.abs(got.astype(np.float64) - r) <= bound), (m, col0, divide)
                    assert np.array_equal(bits(got), bits(w)), (m, col0, divide)


def test_seg_sum_on_a_built_index_reads_the_points_in_place():
    for width in (4, 6, 7):
        pts, t, idx = hot_cloud_index(width, seed=width)
        table = (idx.seg_off.cpu().numpy(), idx.seg_pts.cpu().numpy())
        rows = idx.rows.cpu().numpy()
        for col0, ncol in ((1, 3), (1, width - 1), (width - 1, 1)):
            for divide in (False, True):
                seg_off, seg_pts = table
                poison((idx.M, ncol))
                got = ops.dyn_seg_sum(t, idx, col0, ncol, rowmap=idx.rows, mean=divide).cpu().numpy()
                assert np.array_equal(bits(got), bits(D.seq_sum_f32(pts, seg_off, seg_pts, rows, col0, ncol, divide)))
        assert torch.equal(ops.dyn_points_mean(t, idx, 1, 3), ops.dyn_seg_sum(t, idx, 1, 3, rowmap=idx.rows, mean=True))


def seg_max_values(rng, k, c):
    """small integers (frequent ties); column 0 all -inf, the last column +inf among finite values, one column of +0.0 / -0.0"""
    x = rng.integers(-2, 3, (k, c)).astype(np.float32)
    x[:, 0] = -np.inf
    if c > 2:
        x[:, 1] = np.where(rng.integers(0, 2, k) > 0, np.float32(0.0), np.float32(-0.0))
    if c > 1:
        x[rng.integers(0, 3, k) == 0, c - 1] = np.inf
    return x


@pytest.mark.parametrize("c", [1, 33, 64, 65])
def test_seg_max_ties_infinities_and_signed_zeros(c):
    rng = np.random.default_rng(100 + c)
    for m in D.grid_tail_ms(c):
        seg_off, seg_pts, inv = D.csr_table(D.mixed_lengths(m, rot=m + 1), seed=m)
        k = int(seg_off[-1])
        x = seg_max_values(rng, k, c)
        want, want_arg = D.seg_max_ref(x, seg_off, seg_pts)
        index = table_index(seg_off, seg_pts, inv)
        poison((m, c))
        poison((m, c), torch.int32, -1)
        xg = dev(x).requires_grad_(True)
        got, arg = ops.dyn_seg_max(xg, index)
        assert np.array_equal(bits(got.detach().cpu().numpy()), bits(want)) and np.array_equal(arg.cpu().numpy(), want_arg), (c, m)
        # backward: gout at the argmax rows, exactly 0.0 everywhere else
        gout = rng.standard_normal((m, c)).astype(np.float32)
        poison((k, c))
        got.backward(dev(gout))
        assert np.array_equal(bits(xg.grad.cpu().numpy()), bits(D.seg_max_bwd_ref(gout, want_arg, k))), (c, m)


def test_seg_max_on_a_built_index():
    pts, t, idx = hot_cloud_index(6, seed=9)
    x = seg_max_values(np.random.default_rng(9), idx.K, 33)
    want, want_arg = D.seg_max_ref(x, idx.seg_off.cpu().numpy(), idx.seg_pts.cpu().numpy())
    poison((idx.M, 33))
    got, arg = ops.dyn_seg_max_raw(dev(x), idx)
    assert np.array_equal(bits(got.cpu().numpy()), bits(want)) and np.array_equal(arg.cpu().numpy(), want_arg)


@pytest.mark.parametrize("c", [1, 33])
def test_gather_concat_forward_exact_and_backward_in_segment_order(c):
    """2 * K * c threads just below, on and above a block; backward: the x half is the gradient's first half, the x_max half its
    second half summed per voxel in seg_pts order"""
    rng = np.random.default_rng(200 + c)
    ks = sorted({255 // (2 * c), -(-256 // (2 * c)), -(-257 // (2 * c)), 4097 + 300})
    for k in ks:
        seg_off, seg_pts, inv = D.csr_table(D.lengths_for_rows(k) if k < 4097 else [4097] + D.lengths_for_rows(k - 4097), seed=k)
        m = len(seg_off) - 1
        index = table_index(seg_off, seg_pts, inv)
        x, xmax = rng.standard_normal((k, c)).astype(np.float32), rng.standard_normal((m, c)).astype(np.float32)
        xg, mg = dev(x).requires_grad_(True), dev(xmax).requires_grad_(True)
        poison((k, 2 * c))
        out = ops.dyn_gather_concat(xg, mg, index)
        assert np.array_equal(bits(out.detach().cpu().numpy()), bits(D.gather_concat_ref(x, xmax, inv))), (c, k)
        g = (rng.standard_normal((k, 2 * c)) * 10).astype(np.float32)
        poison((m, c))
        out.backward(dev(g))
        assert np.array_equal(bits(xg.grad.cpu().numpy()), bits(g[:, :c]))
        assert np.array_equal(bits(mg.grad.cpu().numpy()), bits(D.seq_sum_f32(g, seg_off, seg_pts, None, c, c, False))), (c, k)


DECORATE_CASES = [(geom, width, use_abs, dist) for geom in ("small", "waymo") for width in (4, 6, 7) for use_abs in (False, True)
                  for dist in (False, True) if geom == "small" or (use_abs and width == 6)]


@pytest.mark.parametrize("geom,width,use_abs,with_dist", DECORATE_CASES)
def test_pillar_decorate_flags_and_widths(geom, width, use_abs, with_dist):
    """all four (use_abs_xyz, with_dist) at widths 4, 6 and 7 (width 4 without absolute xyz copies no column: f = 6 or 7), a hot pillar
    and single-point pillars, output rows poisoned.  fp64 reference; bound 1e-6 * max(1, |ref|max) as in test_gpu_dyn_vfe.py.  The
    pillar centre cx * vx + x_off is rounded at the size of the coordinate, so without the absolute columns the bound only holds on a
    grid of a few cells: the Waymo range runs with them."""
    pc_range, vs = D.WORD_GRID if geom == "small" else D.WAYMO_PILLAR
    pts = D.decorate_cloud(pc_range, vs, width, seed=width, n=3000 if geom == "waymo" else 60)
    t = dev(pts)
    idx = ops.dyn_voxel_index(t, pc_range, vs, 2, True)
    assert int(idx.cnt.max()) >= 4097 and int((idx.cnt == 1).sum()) >= 1
    mean = ops.dyn_points_mean(t, idx, 1, 3)
    offsets = [vs[j] / 2 + pc_range[j] for j in range(3)]
    f = width - (1 if use_abs else 4) + 6 + int(with_dist)
    poison((idx.K, f))
    got = ops.dyn_pillar_decorate(t, idx, mean, vs, offsets, use_abs, with_dist)
    assert got.shape == (idx.K, f)
    ref = D.decorate_ref64(pts, idx.rows.cpu().numpy(), idx.inv.cpu().numpy(), idx.coords.cpu().numpy(), mean.cpu().numpy(), vs, offsets,
                           use_abs, with_dist)
    err = np.abs(got.cpu().double().numpy() - ref)
    assert not np.isnan(err).any() and err.max() <= 1e-6 * max(1.0, np.abs(ref).max()), err.max()
    # the copied columns are copies
    ncopy = width - (1 if use_abs else 4)
    assert np.array_equal(bits(got[:, :ncopy].cpu().numpy()), bits(pts[idx.rows.cpu().numpy()][:, width - ncopy:]))


def test_empty_index_goes_through_every_wrapper():
    """M = 0 and K = 0: no launch error, correctly shaped empty tensors, gradients included"""
    for pts in (np.zeros((0, 6), np.float32), np.full((70, 6), 500.0, np.float32)):
        t = dev(pts)
        idx = ops.dyn_voxel_index(t, *D.WAYMO_PILLAR, 2, True)
        assert idx.M == 0 and idx.K == 0 and idx.keep.shape == (len(pts),) and not bool(idx.keep.any())
        assert idx.rows.shape == (0,) and idx.inv.shape == (0,) and idx.seg_pts.shape == (0,) and idx.cnt.shape == (0,)
        assert idx.coords.shape == (0, 4) and idx.seg_off.cpu().tolist() == [0]
        mean = ops.dyn_points_mean(t, idx, 1, 3)
        assert mean.shape == (0, 3) and ops.dyn_points_mean(t, idx, 1).shape == (0, 5)
        assert ops.dyn_seg_sum(torch.zeros((0, 8), device=DEV), idx, 2, 3).shape == (0, 3)
        for use_abs in (False, True):
            for dist in (False, True):
                deco = ops.dyn_pillar_decorate(t, idx, mean, D.WAYMO_PILLAR[1], [0.1, 0.2, 0.3], use_abs, dist)
                assert deco.shape == (0, 6 - (1 if use_abs else 4) + 6 + int(dist))
        x = torch.zeros((0, 33), device=DEV, requires_grad=True)
        xmax, arg = ops.dyn_seg_max(x, idx)
        assert xmax.shape == (0, 33) and arg.shape == (0, 33) and arg.dtype == torch.int32
        out = ops.dyn_gather_concat(x, xmax, idx)
        assert out.shape == (0, 66)
        out.sum().backward()
        assert x.grad.shape == (0, 33)
        torch.cuda.synchronize()
