"""Dynamic voxelisation on the MI355X (csrc/dynvox.hip through the C ABI): the index is bit-exact against CPU torch.unique, the
segmented reductions match fp64, DynPillarVFE forward / backward matches the CPU restatement, everything is bit-reproducible, and
both dynamic CenterPoint configurations train a step through the input pipeline."""
import copy
import os

import numpy as np
import pytest
import torch

from toda_amd import ops
from toda_amd.pcdet.models.backbones_3d.vfe.dynamic_pillar_vfe import torch_dyn_index

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WAYMO_PILLAR = ([-74.88, -74.88, -2.0, 74.88, 74.88, 4.0], [0.32, 0.32, 6.0])
WAYMO_VOXEL = ([-75.2, -75.2, -2.0, 75.2, 75.2, 4.0], [0.1, 0.1, 0.15])


def waymo_points(rng, counts, pc_range, c=5):
    """Collated [sum N, 1 + c] clouds: most points in range (a ring-shaped density like a lidar sweep), some outside."""
    parts = []
    for b, n in enumerate(counts):
        p = np.zeros((n, 1 + c), np.float32)
        p[:, 0] = b
        r = np.abs(rng.normal(0, 25, n)) + 2.0
        a = rng.uniform(-np.pi, np.pi, n)
        p[:, 1], p[:, 2] = r * np.cos(a), r * np.sin(a)
        p[:, 3] = rng.uniform(pc_range[2] - 0.5, pc_range[5] + 0.5, n)
        p[:, 4:] = rng.uniform(0, 1, (n, c - 3))
        parts.append(p)
    return np.concatenate(parts) if parts else np.zeros((0, 1 + c), np.float32)


def check_index(pts, pc_range, vs, bs, pillar):
    grid = ops.grid_size_xyz(pc_range, vs)
    t = torch.from_numpy(pts)
    keep, inv, cnt, coords, _ = torch_dyn_index(t, pc_range, vs, grid, bs, pillar)
    idx = ops.dyn_voxel_index(t.cuda(), pc_range, vs, bs, pillar)
    torch.cuda.synchronize()
    assert torch.equal(idx.keep.cpu(), keep)
    assert torch.equal(idx.rows.cpu().long(), torch.nonzero(keep).view(-1))
    assert torch.equal(idx.inv.cpu().long(), inv)
    assert torch.equal(idx.cnt.cpu(), cnt)
    assert torch.equal(idx.coords.cpu(), coords)
    off, segp = idx.seg_off.cpu().long(), idx.seg_pts.cpu().long()
    assert off[0] == 0 and off[-1] == idx.K and torch.equal(off[1:] - off[:-1], cnt.long())
    # each segment: exactly the rows of its voxel, ascending
    order = torch.argsort(inv * (idx.K + 1) + torch.arange(idx.K), stable=True)
    assert torch.equal(segp, order)
    return idx


@pytest.mark.parametrize("pillar", [True, False])
def test_index_full_size_waymo(pillar):
    pc_range, vs = WAYMO_PILLAR if pillar else WAYMO_VOXEL
    pts = waymo_points(np.random.default_rng(0), [180000, 180000], pc_range)
    idx = check_index(pts, pc_range, vs, 2, pillar)
    assert idx.M > 10000


@pytest.mark.parametrize("pillar", [True, False])
def test_index_bounds_nan_outside_empty_sample(pillar):
    pc_range, vs = [-8.0, -8.0, -2.0, 8.0, 8.0, 4.0], ([0.32, 0.32, 6.0] if pillar else [0.1, 0.1, 0.15])
    rng = np.random.default_rng(1)
    a = waymo_points(rng, [3000], pc_range)
    a[:, 1:3] = rng.uniform(-9, 9, (3000, 2))
    b = waymo_points(rng, [3000], pc_range)
    b[:, 0] = 2                                              # sample 1 of the batch is empty
    b[:, 1:3] = rng.uniform(-9, 9, (3000, 2))
    lo, hi = np.asarray(pc_range[:3], np.float32), np.asarray(pc_range[3:], np.float32)
    for j in range(3):                                       # exactly on the lower and upper bounds
        a[10 + j, 1 + j], a[20 + j, 1 + j] = lo[j], hi[j]
        b[10 + j, 1 + j], b[20 + j, 1 + j] = lo[j], hi[j]
    a[30:40, 1] = np.nan
    a[40:45, 3] = np.nan                                    # z NaN: kept by the pillar test (x, y only), dropped by the voxel one
    b[50:60, 2] = 1e9
    pts = np.concatenate([a, b])
    check_index(pts, pc_range, vs, 3, pillar)


def test_index_hot_cell_and_batch_sizes():
    pc_range, vs = WAYMO_PILLAR
    rng = np.random.default_rng(2)
    pts = waymo_points(rng, [70000, 20000], pc_range)
    pts[5:60005, 1:4] = [0.05, 0.05, 0.1]                    # 60 k points in one cell
    idx = check_index(pts, pc_range, vs, 2, True)
    assert int(idx.cnt.max()) >= 60000
    for bs in (1, 2, 16):
        counts = [int(v) for v in rng.integers(1000, 12000, bs)]
        check_index(waymo_points(rng, counts, pc_range), pc_range, vs, bs, True)
        check_index(waymo_points(rng, counts, WAYMO_VOXEL[0]), *WAYMO_VOXEL, bs, False)


def test_index_empty_batch():
    pc_range, vs = WAYMO_PILLAR
    pts = np.full((100, 6), 500.0, np.float32)
    pts[:, 0] = 0
    idx = ops.dyn_voxel_index(torch.from_numpy(pts).cuda(), pc_range, vs, 1, True)
    assert idx.M == 0 and idx.K == 0 and not bool(idx.keep.any())


def test_segment_mean_decoration_and_max():
    from toda_amd.pcdet.config import AttrDict
    from toda_amd.pcdet.models.backbones_3d.vfe import __all__ as vfes

    pc_range, vs = WAYMO_PILLAR
    rng = np.random.default_rng(3)
    pts = waymo_points(rng, [50000, 40000], pc_range)
    pts[7:5007, 1:4] = rng.normal(0, 0.01, (5000, 3)) + [0.1, 0.1, 0.5]      # a hot pillar
    t = torch.from_numpy(pts)
    idx = ops.dyn_voxel_index(t.cuda(), pc_range, vs, 2, True)
    grid = ops.grid_size_xyz(pc_range, vs)
    keep, inv, cnt, coords, cell = torch_dyn_index(t, pc_range, vs, grid, 2, True)
    kept = pts[keep.numpy()].astype(np.float64)
    inv_np, m = inv.numpy(), idx.M
    # mean of every feature column (DynMeanVFE's forward) and of xyz
    mean = np.zeros((m, 5))
    np.add.at(mean, inv_np, kept[:, 1:])
    mean /= cnt.numpy()[:, None]
    got = ops.dyn_points_mean(t.cuda(), idx, 1).cpu().double().numpy()
    assert np.abs(got - mean).max() <= 1e-6 * max(1.0, np.abs(mean).max())
    xyz_mean = ops.dyn_points_mean(t.cuda(), idx, 1, 3)
    # decoration against the fp64 statement
    cfg = AttrDict({"NAME": "DynPillarVFE", "WITH_DISTANCE": True, "USE_ABSLOTE_XYZ": True, "USE_NORM": True, "NUM_FILTERS": [64, 64]})
    vfe = vfes["DynPillarVFE"](model_cfg=cfg, num_point_features=5, voxel_size=vs, grid_size=grid, point_cloud_range=pc_range)
    deco = ops.dyn_pillar_decorate(t.cuda(), idx, xyz_mean, vs, [vfe.x_offset, vfe.y_offset, vfe.z_offset], True, True).cpu().double().numpy()
    xyz = kept[:, 1:4]
    c = cell.numpy()
    ref = np.concatenate([kept[:, 1:], xyz - mean[inv_np, :3],
                          np.stack([xyz[:, 0] - (c[:, 0] * vs[0] + vfe.x_offset), xyz[:, 1] - (c[:, 1] * vs[1] + vfe.y_offset),
                                    xyz[:, 2] - vfe.z_offset], 1), np.linalg.norm(xyz, axis=1, keepdims=True)], 1)
    assert deco.shape == ref.shape
    assert np.abs(deco - ref).max() <= 1e-6 * max(1.0, np.abs(ref).max())
    # segmented max with ties: small integers, the lowest row must win
    x = torch.from_numpy(rng.integers(0, 4, (idx.K, 32)).astype(np.float32))
    xmax, arg = ops.dyn_seg_max_raw(x.cuda(), idx)
    xn = x.numpy()
    order = np.lexsort((np.arange(idx.K), inv_np))                              # rows grouped by voxel, ascending
    ref_max = np.full((m, 32), -np.inf, np.float32)
    ref_arg = np.full((m, 32), -1, np.int64)
    for r in order:
        v = inv_np[r]
        better = xn[r] > ref_max[v]
        ref_max[v] = np.where(better, xn[r], ref_max[v])
        ref_arg[v] = np.where(better, r, ref_arg[v])
    assert np.array_equal(xmax.cpu().numpy(), ref_max) and np.array_equal(arg.cpu().numpy(), ref_arg)
    # its backward and the gather-concat backward
    g = torch.from_numpy(rng.standard_normal((m, 32)).astype(np.float32))
    xg = x.cuda().requires_grad_(True)
    ops.dyn_seg_max(xg, idx)[0].backward(g.cuda())
    ref_gx = np.zeros((idx.K, 32), np.float32)
    ref_gx[ref_arg, np.arange(32)[None, :]] = g.numpy()
    assert np.array_equal(xg.grad.cpu().numpy(), ref_gx)
    xg.grad = None
    xm = torch.from_numpy(ref_max).cuda().requires_grad_(True)
    out = ops.dyn_gather_concat(xg, xm, idx)
    assert torch.equal(out.detach().cpu(), torch.cat([x, torch.from_numpy(ref_max)[inv]], 1))
    go = torch.from_numpy(rng.standard_normal((idx.K, 64)).astype(np.float32))
    out.backward(go.cuda())
    ref_gm = np.zeros((m, 32))
    np.add.at(ref_gm, inv_np, go.numpy()[:, 32:].astype(np.float64))
    assert torch.equal(xg.grad.cpu(), go[:, :32])
    assert np.abs(xm.grad.cpu().double().numpy() - ref_gm).max() <= 1e-5 * max(1.0, np.abs(ref_gm).max())


def _pillar_vfe(pc_range, vs, seed=0):
    from toda_amd.pcdet.config import AttrDict
    from toda_amd.pcdet.models.backbones_3d.vfe import __all__ as vfes

    cfg = AttrDict({"NAME": "DynPillarVFE", "WITH_DISTANCE": False, "USE_ABSLOTE_XYZ": True, "USE_NORM": True, "NUM_FILTERS": [64, 64]})
    torch.manual_seed(seed)
    vfe = vfes["DynPillarVFE"](model_cfg=cfg, num_point_features=5, voxel_size=vs, grid_size=ops.grid_size_xyz(pc_range, vs),
                               point_cloud_range=pc_range)
    for layer in vfe.pfn_layers:          # non-trivial affine parameters
        layer.norm.weight.data.uniform_(0.5, 1.5)
        layer.norm.bias.data.uniform_(-0.2, 0.2)
    return vfe.train()


def _run_pfn(vfe, feats, index, gout):
    """PFN stack on leaf features; returns (output, grad of the features, grads of every parameter)."""
    f = feats.detach().clone().requires_grad_(True)
    x = f
    for pfn in vfe.pfn_layers:
        x = pfn(x, index)
    x.backward(gout)
    grads = [p.grad.detach().clone() for p in vfe.parameters()]
    vfe.zero_grad(set_to_none=True)
    return x.detach(), f.grad.detach(), grads


def test_dyn_pillar_vfe_fwd_bwd_matches_cpu_fp64_and_is_reproducible():
    pc_range, vs = [-20.48, -20.48, -2.0, 20.48, 20.48, 4.0], [0.32, 0.32, 6.0]
    rng = np.random.default_rng(4)
    pts = waymo_points(rng, [6000, 5000], pc_range)
    pts[:, 1:3] = rng.uniform(-21, 21, (11000, 2))
    t = torch.from_numpy(pts)
    vfe = _pillar_vfe(pc_range, vs)
    cpu = copy.deepcopy(vfe).double()
    gpu = copy.deepcopy(vfe).cuda()
    idx = ops.dyn_voxel_index(t.cuda(), pc_range, vs, 2, True)
    keep, inv, cnt, coords, cell = torch_dyn_index(t, pc_range, vs, ops.grid_size_xyz(pc_range, vs), 2, True)
    assert torch.equal(idx.inv.cpu().long(), inv)
    # decoration
    mean = ops.dyn_points_mean(t.cuda(), idx, 1, 3)
    deco = ops.dyn_pillar_decorate(t.cuda(), idx, mean, vs, [vfe.x_offset, vfe.y_offset, vfe.z_offset], True, False)
    deco_ref = cpu.decorate_torch(t.double(), keep, inv, cell, idx.M)
    assert float((deco.cpu().double() - deco_ref).abs().max()) <= 1e-5
    gout = torch.from_numpy(rng.standard_normal((idx.M, 64)))
    y0, gf0, gp0 = _run_pfn(cpu, deco_ref, (inv, idx.M), gout)
    y1, gf1, gp1 = _run_pfn(gpu, deco_ref.float().cuda(), idx, gout.float().cuda())

    def rel(a, b):
        return float((a.cpu().double() - b).abs().max()) / max(1.0, float(b.abs().max()))

    assert rel(y1, y0) < 1e-5
    assert rel(gf1, gf0) < 1e-4
    assert len(gp1) == 6 and all(rel(a, b) < 1e-4 for a, b in zip(gp1, gp0))
    # the whole module forward, and bit reproducibility of a second run (new index, same kernels)
    out = [gpu({"points": t.cuda(), "batch_size": 2})["pillar_features"].detach() for _ in range(2)]
    assert torch.equal(out[0], out[1])
    idx2 = ops.dyn_voxel_index(t.cuda(), pc_range, vs, 2, True)
    for a in ("keep", "rows", "inv", "cnt", "coords", "seg_off", "seg_pts"):
        assert torch.equal(getattr(idx, a), getattr(idx2, a)), a
    y2, gf2, gp2 = _run_pfn(gpu, deco_ref.float().cuda(), idx2, gout.float().cuda())
    assert torch.equal(y1, y2) and torch.equal(gf1, gf2) and all(torch.equal(a, b) for a, b in zip(gp1, gp2))


def _small_cfg(name, rng_xy, n_points):
    from toda_amd.pcdet.config import AttrDict, cfg_from_yaml_file

    cfg = AttrDict()
    cfg_from_yaml_file(os.path.join(ROOT, "toda_amd/tools/cfgs/models/{}.yaml".format(name)), cfg)
    r = cfg.DATA_CONFIG.POINT_CLOUD_RANGE
    cfg.DATA_CONFIG.POINT_CLOUD_RANGE = [-rng_xy, -rng_xy, r[2], rng_xy, rng_xy, r[5]]
    cfg.DATA_CONFIG.SYNTHETIC.NUM_POINTS = n_points
    cfg.MODEL.DENSE_HEAD.POST_PROCESSING.POST_CENTER_LIMIT_RANGE = [-rng_xy, -rng_xy, -10, rng_xy, rng_xy, 10]
    return cfg


@pytest.mark.parametrize("name,rng_xy", [("centerpoint_dyn_pillar_waymo", 16.0), ("centerpoint_dyn_voxel_waymo", 16.0)])
def test_training_step_through_input_prefetcher_matches_cpu(name, rng_xy):
    from oracle.cpu_backend import oracle_backend
    from toda_amd.pcdet.datasets import SyntheticLidarDataset
    from toda_amd.pcdet.models import InputPrefetcher, build_network, model_fn_decorator

    cfg = _small_cfg(name, rng_xy, 12000)
    ds = SyntheticLidarDataset(cfg.DATA_CONFIG, cfg.CLASS_NAMES)
    torch.manual_seed(0)
    cpu_model = build_network(cfg.MODEL, len(cfg.CLASS_NAMES), ds).train()
    gpu_model = copy.deepcopy(cpu_model).cuda()
    batch = ds.collate_batch([ds[0], ds[1]])
    bev = {}

    def hook(tag):
        def _h(_m, _a, out):
            bev[tag] = out["spatial_features_2d"].detach().cpu()
        return _h

    h0 = cpu_model.backbone_2d.register_forward_hook(hook("cpu"))
    h1 = gpu_model.backbone_2d.register_forward_hook(hook("gpu"))
    with oracle_backend():
        ref = model_fn_decorator()(cpu_model, {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in batch.items()})
        ref.loss.backward()
    pre = InputPrefetcher(iter([{k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in batch.items()}]), gpu_model,
                          torch.device("cuda", 0))
    try:
        b = pre.next()
        assert "voxels" not in b
        assert isinstance(b.get("dyn_voxel_index"), ops.DynVoxelIndex) and b["voxel_coords"] is b["dyn_voxel_index"].coords
        if name.endswith("voxel_waymo"):
            assert "sparse_index_plan" in b          # the rulebooks were built on the side stream too
        ret, tb, _ = gpu_model(b)
        loss = ret["loss"].mean()
        loss.backward()
    finally:
        pre.close()
        h0.remove()
        h1.remove()
    assert abs(float(loss) - float(ref.loss)) <= 1e-3 * max(1.0, abs(float(ref.loss)))
    d = float((bev["gpu"] - bev["cpu"]).abs().max()) / max(1.0, float(bev["cpu"].abs().max()))
    assert d <= 1e-3, d
    assert all(torch.isfinite(p.grad).all() for p in gpu_model.parameters() if p.grad is not None)
