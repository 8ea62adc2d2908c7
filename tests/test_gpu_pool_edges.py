"""The two-stage heads' query and pool kernels (csrc/roi_head.hip, voxel_pool.hip, pointnet2_stack.hip) at the shapes where their
code paths change: gt tiles of the IoU max, channel chunks and grid sizes of the RoI grid pool, the fused voxel pool's point groups
and channel lanes, the FPS host split and workgroup crossovers, the ball query's radius count and nsample bounds, channel and
nsample tails of the SA gather / max, and samples without points or queries in the middle of a batch.  Each kernel is held to
the suite's references: exact for index outputs, the existing relative bounds against fp64 for values."""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from toda_amd import ops
from toda_amd.pcdet.models.backbones_3d.pfe.voxel_set_abstraction import bilinear_interpolate_torch
from toda_amd.pcdet.models.roi_heads.second_head import roi_grid_pool_torch
from toda_amd.pcdet.ops.pointnet2.pointnet2_stack import pointnet2_utils
from toda_amd.pcdet.ops.pointnet2.pointnet2_stack.voxel_pool_modules import folded_position_map, pool_torch
from toda_amd.pcdet.ops.pointnet2.pointnet2_stack.voxel_query_utils import VoxelLevel, voxel_query_torch
from toda_amd.pcdet.utils.common_utils import get_voxel_centers

from tests.test_gpu_pv_rcnn import ball_query_restated, cloud, fps_restated
from tests.test_gpu_second_iou import _expected, _iou_case
from tests.test_gpu_voxel_rcnn import PC_RANGE, VSIZE, assert_margin, bound, coords_of, grid_points, make_level, pool_inputs, ref64

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)


def poison(shape, dtype=torch.float32, value=float("nan")):
    """Leave a block of this size filled with `value` in torch's caching allocator: the next output of that size usually lands in
    it, so an element a kernel never writes reads as NaN (or -1) instead of an earlier, correct result."""
    torch.full(shape, value, dtype=dtype, device=DEV)


# ------------------------------------------------------------------------------------------------------------------ roi_head.hip
@pytest.mark.parametrize("by_class", [True, False])
def test_roi_iou3d_max_across_gt_tiles(by_class):
    """255, 256, 257 and 700 valid gts (IOU_TILE = 256 per LDS tile); the same box in tile 0 and tile 2; class-3 gts only past
    tile 0; zero rows inside the valid range of later tiles."""
    rng = np.random.default_rng(31 if by_class else 32)
    rois, labels, gt = _iou_case(rng, 4, 512, 720, [255, 256, 257, 700])
    gt[3, :256, 7] = rng.integers(1, 3, 256)            # sample 3: no class-3 gt in tile 0 ...
    gt[3, 256:700:3, 7] = 3                             # ... plenty in tiles 1 and 2
    gt[3, 600] = gt[3, 5]                               # one box in tile 0 and again in tile 2: the lower index wins
    rois[3, 0], labels[3, 0] = gt[3, 5, :7], int(gt[3, 5, 7])
    rois[2, 0], labels[2, 0] = gt[2, 256, :7], int(gt[2, 256, 7])     # the one gt of sample 2's second tile
    gt[3, 300] = 0                                      # zero rows inside the valid range of tiles 1 and 2
    gt[3, 520] = 0
    want_iou, want_idx = _expected(rois, labels, gt, by_class)
    iou, idx = ops.roi_iou3d_max(torch.from_numpy(rois).to(DEV), torch.from_numpy(labels).to(DEV), torch.from_numpy(gt).to(DEV), by_class)
    iou, idx = iou.cpu().numpy(), idx.cpu().numpy()
    np.testing.assert_allclose(iou, want_iou, rtol=0, atol=1e-5)
    pos = want_iou > 1e-4
    np.testing.assert_array_equal(idx[pos], want_idx[pos])
    assert abs(float(iou[3, 0]) - 1.0) < 1e-4 and int(idx[3, 0]) == 5
    assert abs(float(iou[2, 0]) - 1.0) < 1e-4 and int(idx[2, 0]) == 256
    for s in range(4):                                  # every sample has rois matched past its first tile, or fills it exactly
        assert (pos[s] & (want_idx[s] >= 200)).sum() > 10
    late = pos[3] & (want_idx[3] >= 256)
    assert late.sum() > 100
    if by_class:                                        # class-3 rois of sample 3: every eligible gt lies in tiles 1 and 2
        c3 = pos[3] & (labels[3] == 3)
        assert c3.sum() > 20 and bool((want_idx[3][c3] >= 256).all())


def _pool_rois(rng, b, n, w, h):
    """Rois in map units of a [h, w] map at 1 m cells from (0, 0): centres on every edge and corner and outside it, headings at
    +-pi and +-pi/2 and at random, sizes up to 1.5 x the map; sample 1 is all zero padding."""
    rois = np.zeros((b, n, 7), np.float32)
    xs, ys = [0.0, w / 2, float(w), -0.7, w + 0.7], [0.0, h / 2, float(h), -0.7, h + 0.7]
    heads = [np.pi, -np.pi, np.pi / 2, -np.pi / 2, 0.0]
    for s in range(b):
        k = 0
        for x in xs:
            for y in ys:
                rois[s, k, 0:2] = (x, y)
                rois[s, k, 6] = heads[k % len(heads)]
                k += 1
        rois[s, k:, 0] = rng.uniform(-1, w + 1, n - k)
        rois[s, k:, 1] = rng.uniform(-1, h + 1, n - k)
        rois[s, k:, 6] = rng.uniform(-np.pi, np.pi, n - k)
        rois[s, :, 2] = rng.uniform(-1, 1, n)
        rois[s, :, 3] = rng.uniform(0.3, 1.5 * w, n)
        rois[s, :, 4] = rng.uniform(0.3, 1.5 * h, n)
        rois[s, :, 5] = rng.uniform(0.5, 2, n)
    if b > 1:
        rois[1] = 0
    return rois


@pytest.mark.parametrize("c,g,h,w", [(1, 1, 2, 3), (31, 16, 2, 3), (33, 16, 5, 4), (65, 1, 9, 7), (65, 16, 3, 2)])
def test_roi_grid_pool_channel_tails_grid_sizes_and_map_edges(c, g, h, w):
    """C around POOL_CHUNK = 32 channels per workgroup, G = 1 and G = 16 (POOL_MAX_CELLS), maps down to 2 x 3, rois straddling
    every edge: against roi_grid_pool_torch in fp64 with the yardstick of the TODA-shape test."""
    rng = np.random.default_rng(c * 100 + g * 10 + h)
    feat = torch.from_numpy(rng.standard_normal((3, c, h, w)).astype(np.float32)).to(DEV)
    rois = torch.from_numpy(_pool_rois(rng, 3, 40, w, h)).to(DEV)
    args = (0.0, 0.0, 0.5, 0.5, 2, g)
    poison((3 * 40, c, g, g))
    a = ops.roi_grid_pool(feat, rois, *args)
    b = ops.roi_grid_pool(feat, rois, *args)
    assert a.shape == (3 * 40, c, g, g) and bool(torch.isfinite(a).all())
    assert torch.equal(a, b)
    ref = roi_grid_pool_torch(feat, rois, *args)
    exact = roi_grid_pool_torch(feat.double(), rois.double(), *args)
    top = float(feat.abs().max())
    assert float((a - ref).abs().max()) <= 1e-4 * top
    err_kernel = float((a.double() - exact).abs().max())
    err_torch = float((ref.double() - exact).abs().max())
    assert err_kernel <= max(1.5 * err_torch, 1e-5 * top), (err_kernel, err_torch)
    assert float(exact.abs().max()) > 0.1


def test_roi_grid_pool_rejects_degenerate_maps_and_grids():
    feat = torch.zeros((1, 4, 1, 5), device=DEV)
    rois = torch.zeros((1, 2, 7), device=DEV)
    with pytest.raises(RuntimeError, match="not supported"):
        ops.roi_grid_pool(feat, rois, 0.0, 0.0, 1.0, 1.0, 1, 2)
    with pytest.raises(RuntimeError, match="grid size"):
        ops.roi_grid_pool(torch.zeros((1, 4, 3, 5), device=DEV), rois, 0.0, 0.0, 1.0, 1.0, 1, 17)


# ---------------------------------------------------------------------------------------------------------------- voxel_pool.hip
def _level_without_sample_1(n, seed):
    shape = [10, 80, 64]
    coords = make_level(3, shape, n, seed, "sorted")
    coords = coords[coords[:, 0] != 1].contiguous()     # sample 1 has no sites at this level
    xyz = get_voxel_centers(coords[:, 1:4], 2, VSIZE, PC_RANGE).contiguous()
    gi = ops.GridIndex.from_coords(coords, 3, shape)
    return coords, xyz, gi, VoxelLevel(coords, shape, 3, gi)


@pytest.mark.parametrize("nsample,m_per", [(1, 1), (64, 1), (1, 17), (64, 17)])
def test_voxel_query_middle_sample_without_sites(nsample, m_per):
    coords, xyz, gi, level = _level_without_sample_1(30000, 61 + nsample)
    lo = [PC_RANGE[j] + 1.0 for j in range(3)]
    hi = [PC_RANGE[3 + j] - 1.0 for j in range(3)]
    new_xyz, bidx = grid_points(3, m_per, lo, hi, 62 + m_per)
    nc = coords_of(new_xyz, bidx, PC_RANGE, VSIZE, 2)
    res = []
    for sel in (slice(None), slice(3 * m_per - 1, None)):             # the batch, then M = 1 (a grid point of sample 2)
        args = (new_xyz[sel].contiguous(), nc[sel].contiguous(), xyz)
        idx, empty = ops.voxel_query(*args, gi, 1.0, (2, 4, 4), nsample)
        idx_t, empty_t = voxel_query_torch(*args, level, 1.0, (2, 4, 4), nsample)
        assert torch.equal(idx, idx_t) and torch.equal(empty, empty_t), sel
        res.append((idx, empty))
    (idx, empty), (idx1, _) = res
    assert idx1.shape == (1, nsample) and torch.equal(idx1[0], idx[-1])
    b = bidx.view(-1).long()
    assert bool(empty[b == 1].all()) and bool((idx[b == 1] == 0).all())
    assert bool((~empty[b == 0]).all()) and bool((~empty[b == 2]).all())
    if nsample == 64 and m_per == 17:
        assert bool((idx[:, 63] != idx[:, 0]).any())                   # a saturated ball: 64 hits


def test_voxel_query_rejects_nsample_past_its_bound():
    coords, xyz, gi, _ = _level_without_sample_1(500, 3)
    new_xyz, bidx = grid_points(3, 2, PC_RANGE[:3], PC_RANGE[3:], 4)
    with pytest.raises(RuntimeError, match="nsample"):
        ops.voxel_query(new_xyz, coords_of(new_xyz, bidx, PC_RANGE, VSIZE, 2), xyz, gi, 1.0, (1, 1, 1), 65)


def _voxel_pool_run(f, idx, empty, xyz, new_xyz, pos, gout):
    pos.zero_grad()
    fk = f.clone().requires_grad_(True)
    a, b = folded_position_map(pos, idx, empty, xyz, new_xyz)
    out = ops.voxel_neighbor_pool(fk, a, b, idx, empty, xyz, new_xyz)
    out.backward(gout)
    return [out.detach(), fk.grad] + [p.grad.clone() for p in pos.parameters()]


@pytest.mark.parametrize("c,radius", [(1, 0.6), (63, 0.6), (65, 0.6), (130, 0.6), (65, 0.0)])
def test_voxel_pool_channel_tails_and_empty_balls(c, radius):
    """C around the 64-channel lanes of d a / d b, M = 74 grid points (not a multiple of VP_POINTS = 16), nsample = 64
    (VP_MAX_NSAMPLE); radius 0 leaves every ball empty.  Forward and backward against the fp64 composition; bit-reproducible."""
    f, idx, empty, xyz, new_xyz, pos = pool_inputs(40 + c, n=3000, m=74, c=c, nsample=64, radius=radius)
    assert idx.shape == (74, 64)
    if radius == 0.0:
        assert bool(empty.all())
    else:
        assert bool(empty.any()) and bool((~empty).any())
    assert_margin(f, idx, empty, xyz, new_xyz, pos)
    gout = torch.randn((74, c), generator=torch.Generator().manual_seed(c)).to(DEV)
    snap = copy.deepcopy(pos.state_dict())
    pos_t = copy.deepcopy(pos)
    want, f64, p64 = ref64(f, idx, empty, xyz, new_xyz, pos)
    want.backward(gout.double())
    ft = f.clone().requires_grad_(True)
    t32 = pool_torch(ft, idx, empty, xyz, new_xyz, pos_t)
    t32.backward(gout)
    runs = []
    for _ in range(2):
        pos.load_state_dict(snap)
        runs.append(_voxel_pool_run(f, idx, empty, xyz, new_xyz, pos, gout))
    assert all(torch.equal(x, y) for x, y in zip(*runs))
    got = runs[0]
    err, tol = bound(got[0], want, t32)
    assert err <= tol, ("out", err, tol)
    pairs = [(got[1], f64.grad, ft.grad)] + list(zip(got[2:], [p.grad for p in p64.parameters()], [p.grad for p in pos_t.parameters()]))
    for k, (g_k, g_64, g_t) in enumerate(pairs):
        err, tol = bound(g_k, g_64, g_t)
        assert err <= tol, (k, err, tol)


# ----------------------------------------------------------------------------------------------------------- pointnet2_stack.hip
def _fps_case(counts, npoint, modes, seed, dup=True):
    """FPS of a stacked batch in every mode, index for index against fps_torch per sample (zeros for an empty sample)."""
    xyz = torch.cat([cloud(c, seed + i, dup=c // 10 if dup else 0) for i, c in enumerate(counts)], 0)
    want = [fps_restated(xyz[s:s + c], npoint) if c else torch.zeros((npoint,), dtype=torch.int64)
            for s, c in zip(np.cumsum([0] + counts[:-1]).tolist(), counts)]
    for mode in modes:
        poison((len(counts), npoint), torch.int32, -1)
        got = ops.farthest_point_sample(xyz.to(DEV), counts, npoint, mode=mode).cpu().long()
        ops.L.check(ops.L.load().toda_device_fault(), "toda_device_fault")
        for b, w in enumerate(want):
            assert torch.equal(got[b], w), (mode, b, counts[b])
    return xyz, want


def test_fps_batch_of_17_crosses_the_host_split():
    """FPS_MAX_B = 16 samples per launch: the 17th goes to a second launch (and, being large, to the workgroup groups in auto
    mode while the first launch runs one workgroup per sample)."""
    counts = [300 + 61 * i for i in range(16)] + [9000]
    _fps_case(counts, 64, (0, 1, 2), 100)


def test_fps_around_the_workgroup_point_counts():
    """FPS_BLOCK x FPS_PPT = 4096 points per workgroup of the group kernel, FPS_MULTI_MIN_POINTS = 8192 for the auto choice."""
    _fps_case([4095, 4096, 4097, 8191, 8192], 200, (0, 1, 2), 200)
    _fps_case([8191], 200, (0,), 210)
    _fps_case([8192], 200, (0,), 220)


def test_fps_npoint_one_and_every_point():
    _fps_case([1, 5, 4097], 1, (0, 1, 2), 300)
    xyz, want = _fps_case([4097], 4097, (0, 1, 2), 310, dup=False)
    assert torch.unique(xyz[want[0]], dim=0).shape == torch.unique(xyz, dim=0).shape     # every distinct position is picked


def test_fps_empty_sample_inside_the_batch():
    counts = [9000, 0, 5000]
    xyz = torch.cat([cloud(c, 400 + i) for i, c in enumerate(counts)], 0).to(DEV)
    with pytest.raises(RuntimeError, match="empty"):
        ops.farthest_point_sample(xyz, counts, 100, mode=2)
    _fps_case(counts, 100, (0, 1), 400, dup=False)                              # auto falls back to one workgroup per sample


@pytest.mark.parametrize("nr", [3, 4])
def test_ball_query_radii_nsample_bounds_and_ragged_batch(nr):
    """3 and 4 radii (BQ_MAX_R) in one scan, nsample 1 and 128 (BQ_MAX_NSAMPLE), radius 0, points at exactly r on the 1/8
    lattice (strict <), a batch of 5 with a sample without points and one without queries."""
    counts, m_per = [700, 0, 350, 900, 41], [300, 120, 0, 250, 64]
    radii, nsamples = [1.5, 0.5, 1.0, 0.0][:nr], [128, 1, 16, 128][:nr]
    xyz = torch.cat([cloud(c, 500 + i, extent=(6.0, 6.0, 2.0), dup=c // 20) for i, c in enumerate(counts)], 0).to(DEV)
    new_xyz = torch.cat([cloud(m, 510 + i, extent=(7.0, 7.0, 2.5)) for i, m in enumerate(m_per)], 0).to(DEV)
    xs, ns_ = np.cumsum([0] + counts).tolist(), np.cumsum([0] + m_per).tolist()
    got = ops.ball_query_stack(radii, nsamples, xyz, ops.batch_starts(counts, DEV), new_xyz, ops.batch_starts(m_per, DEV))
    for (idx, empty), r, ns in zip(got, radii, nsamples):
        want_idx, want_empty = ball_query_restated(r, ns, xyz, xs, new_xyz, ns_)
        assert torch.equal(empty, want_empty) and torch.equal(idx, want_idx), (r, ns)
        assert bool(empty[ns_[1]:ns_[2]].all())                                # the sample without points
        if r == 0.0:
            assert bool(empty.all()) and not bool(idx.any())
        else:
            assert bool((~empty).any())
    assert bool((got[0][0][:, 127] != got[0][0][:, 0]).any())                   # a ball with >= 128 hits
    q, p = new_xyz[:m_per[0]], xyz[:counts[0]]
    d2 = ((q[:, None, :] - p[None]) ** 2).sum(-1)                               # exact on the 1/8 lattice
    assert int((d2 == 0.25).sum()) > 0 and int((d2 == 1.0).sum()) > 0           # pairs at exactly r = 0.5 and r = 1


def test_ball_query_rejects_radius_count_and_nsample_past_their_bounds():
    xyz = cloud(100, 1).to(DEV)
    st = ops.batch_starts([100], DEV)
    with pytest.raises(RuntimeError, match="radii"):
        ops.ball_query_stack([1.0] * 5, [4] * 5, xyz, st, xyz, st)
    for ns in (0, 129):
        with pytest.raises(RuntimeError, match="nsample"):
            ops.ball_query_stack([1.0], [ns], xyz, st, xyz, st)


def _lattice(shape, scale, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-64, 65, shape, generator=g).float() / scale


def _sa_case(c, ns, radius, m_per, seed):
    """Points and queries on the 1/8 lattice with duplicated points (and duplicated features), P and wd on coarse lattices: every
    z = P[idx] + wd . d is exact in fp32, so the max has the same (exact) ties in the kernel and in fp64."""
    counts = [400, 0, 300]                                                      # the middle sample has no points
    xyz, feats = [], []
    for i, n in enumerate(counts):
        xyz.append(cloud(n, seed + i, extent=(5.0, 5.0, 2.0), dup=n // 4))
        f = _lattice((n, c), 16, seed + 20 + i)
        f[n - n // 4:] = f[:n // 4]
        feats.append(f)
    xyz, P = torch.cat(xyz, 0), torch.cat(feats, 0)
    new_xyz = torch.cat([cloud(m, seed + 10 + i, extent=(6.0, 6.0, 2.5)) for i, m in enumerate(m_per)], 0)
    ((idx, empty),) = ops.ball_query_stack([radius], [ns], xyz.to(DEV), ops.batch_starts(counts, DEV), new_xyz.to(DEV),
                                           ops.batch_starts(m_per, DEV))
    return xyz, new_xyz, P, _lattice((c, 3), 64, seed + 30), idx, empty


def _sa_run(xyz, new_xyz, P, wd, idx, empty, gout):
    Pk, wk = P.to(DEV).requires_grad_(True), wd.to(DEV).requires_grad_(True)
    z = ops.sa_gather(Pk, wk, idx, empty, xyz.to(DEV), new_xyz.to(DEV))
    out = ops.sa_max(z, idx.shape[0], idx.shape[1])
    out.backward(gout.to(DEV))
    return out.detach().cpu(), Pk.grad.cpu(), wk.grad.cpu()


def _rel(got, want):
    return float((got.double() - want).abs().max()) / max(float(want.abs().max()), 1e-6)


@pytest.mark.parametrize("c,ns,radius", [(1, 1, 1.0), (3, 64, 1.0), (65, 128, 1.0), (65, 1, 1.0), (1, 128, 1.0), (3, 64, 0.0)])
def test_sa_gather_and_max_channel_nsample_tails_and_ties(c, ns, radius):
    """The SA pool's gather + max (no ReLU between them, so maxima of either sign) against the fp64 composition QueryAndGroup.group
    -> Conv2d 1 x 1 -> F.max_pool2d, forward and backward; radius 0 leaves every ball empty."""
    xyz, new_xyz, P, wd, idx, empty = _sa_case(c, ns, radius, [37, 20, 11], 600 + c + ns)
    m = idx.shape[0]
    gout = torch.randn((m, c), generator=torch.Generator().manual_seed(ns))
    out, gP, gwd = _sa_run(xyz, new_xyz, P, wd, idx, empty, gout)
    P64, wd64 = P.double().requires_grad_(True), wd.double().requires_grad_(True)
    grouped = pointnet2_utils.QueryAndGroup.group(xyz.double(), new_xyz.double(), P64, idx.cpu(), empty.cpu(), True)   # (M, 3 + C, ns)
    w = torch.cat([wd64, torch.eye(c, dtype=torch.float64)], 1).view(c, 3 + c, 1, 1)
    y = F.conv2d(grouped.permute(1, 0, 2).unsqueeze(0), w)
    want = F.max_pool2d(y, kernel_size=[1, y.size(3)]).squeeze(-1).squeeze(0).permute(1, 0)
    want.backward(gout.double())
    assert _rel(out, want.detach()) < 2e-5
    assert _rel(gP, P64.grad) < 1e-4 and _rel(gwd, wd64.grad) < 1e-4
    e = empty.cpu()
    assert bool(e[37:57].all())                                                 # queries of the sample without points
    if radius == 0.0:
        assert bool(e.all()) and not bool(gP.any()) and not bool(gwd.any())
    else:
        assert bool((~e).any()) and bool((want[~e] < 0).any())                  # negative maxima pass their gradient too


def test_sa_gather_and_max_without_queries():
    xyz, new_xyz, P, wd, idx, empty = _sa_case(65, 64, 1.0, [0, 0, 0], 700)
    assert idx.shape == (0, 64)
    out, gP, gwd = _sa_run(xyz, new_xyz, P, wd, idx, empty, torch.zeros((0, 65)))
    assert out.shape == (0, 65)
    assert gP.shape == P.shape and not bool(gP.any()) and not bool(gwd.any())


@pytest.mark.parametrize("ns", [1, 7, 254])
def test_sa_max_gradient_matches_max_pool2d_for_negative_maxima_and_ties_at_zero(ns):
    """ops.sa_max is F.max_pool2d over nsample whatever the sign of the maximum: the gradient goes to the first arg-max."""
    m, c = 45, 5
    y = _lattice((m, ns, c), 8, ns)                                             # coarse values: exact ties
    y[:15] = -y[:15].abs() - 0.125                                              # negative maxima
    y[15:30] = -y[15:30].abs()                                                  # maxima at 0 ...
    y[15:30, ns // 2] = 0.0                                                     # ... tied wherever another entry is 0 too
    gout = torch.randn((m, c), generator=torch.Generator().manual_seed(ns))
    yk = y.view(m * ns, c).to(DEV).requires_grad_(True)
    out = ops.sa_max(yk, m, ns)
    out.backward(gout.to(DEV))
    y64 = y.double().permute(2, 0, 1).unsqueeze(0).contiguous().requires_grad_(True)   # (1, C, M, ns)
    want = F.max_pool2d(y64, kernel_size=[1, ns]).squeeze(-1).squeeze(0).permute(1, 0)
    want.backward(gout.double())
    assert torch.equal(out.detach().cpu().double(), want.detach())
    assert torch.equal(yk.grad.cpu().double().view(m, ns, c), y64.grad.squeeze(0).permute(1, 2, 0))
    assert bool((want[:15] < 0).all()) and bool((want[15:30] == 0).all())


def test_sa_max_rejects_nsample_past_its_byte():
    with pytest.raises(RuntimeError, match="nsample"):
        ops.sa_max(torch.zeros((2 * 255, 3), device=DEV), 2, 255)


def test_bev_interpolation_empty_middle_sample_and_edge_keypoints():
    """A batch of 3 whose middle sample has no keypoints; keypoints on every integer pixel, at W - 1 / H - 1 and beyond the map;
    then K = 0.  Forward and backward against fp64, forward bit-exact against fp32 torch."""
    g = torch.Generator().manual_seed(8)
    b, c, h, w = 3, 6, 5, 7
    fmap = torch.randn((b, c, h, w), generator=g)
    yi, xi = torch.meshgrid(torch.arange(h).float(), torch.arange(w).float(), indexing="ij")
    x0 = torch.cat([xi.reshape(-1), torch.tensor([w - 1.0, w - 1.0, 0.5, w - 1.0, w - 1.5]), torch.rand((20,), generator=g) * (w + 3) - 1.5])
    y0 = torch.cat([yi.reshape(-1), torch.tensor([h - 1.0, 0.25, h - 1.0, h - 1.5, h - 1.0]), torch.rand((20,), generator=g) * (h + 3) - 1.5])
    x2 = torch.cat([torch.randint(0, w, (15,), generator=g).float(), torch.rand((25,), generator=g) * (w + 3) - 1.5])
    y2 = torch.cat([torch.randint(0, h, (15,), generator=g).float(), torch.rand((25,), generator=g) * (h + 3) - 1.5])
    x, y = torch.cat([x0, x2]), torch.cat([y0, y2])
    bidx = torch.cat([torch.zeros(len(x0), dtype=torch.int32), torch.full((len(x2),), 2, dtype=torch.int32)])
    fm = fmap.to(DEV).requires_grad_(True)
    out = ops.bev_interpolate(fm, x.to(DEV), y.to(DEV), bidx.to(DEV))
    gout = torch.randn(out.shape, generator=g)
    out.backward(gout.to(DEV))
    f64 = fmap.double().requires_grad_(True)
    want = torch.cat([bilinear_interpolate_torch(f64[s].permute(1, 2, 0), x[bidx == s].double(), y[bidx == s].double()) for s in range(b)])
    want.backward(gout.double())
    want = want.detach()
    assert float((out.detach().cpu().double() - want).abs().max()) < 1e-5 * float(want.abs().max())
    assert float((fm.grad.cpu().double() - f64.grad).abs().max()) < 1e-5 * float(f64.grad.abs().max())
    assert not bool(fm.grad[1].any())
    want32 = torch.cat([bilinear_interpolate_torch(fmap[s].permute(1, 2, 0), x[bidx == s], y[bidx == s]) for s in range(b)])
    assert torch.equal(out.detach().cpu(), want32)

    fk = fmap.to(DEV).requires_grad_(True)
    none = torch.zeros((0,), device=DEV)
    out = ops.bev_interpolate(fk, none, none, torch.zeros((0,), dtype=torch.int32, device=DEV))
    assert out.shape == (0, c)
    out.backward(torch.zeros((0, c), device=DEV))
    assert fk.grad is None or not bool(fk.grad.any())
