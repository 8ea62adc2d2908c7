"""Voxel R-CNN on the MI355X: the HIP voxel query against its torch restatement (exact), the fused neighbour pool forward and
backward against an fp64 evaluation of the reference's composition, BatchNorm2d running statistics, reproducibility, and both
configurations training and evaluating."""
import copy

import numpy as np
import pytest
import torch

from toda_amd import ops
from toda_amd.pcdet.ops.pointnet2.pointnet2_stack.voxel_pool_modules import NeighborVoxelSAModuleMSG, folded_position_map, pool_torch
from toda_amd.pcdet.ops.pointnet2.pointnet2_stack.voxel_query_utils import VoxelLevel, voxel_query_torch
from toda_amd.pcdet.utils.common_utils import get_voxel_centers

from tests.test_voxel_rcnn_host import load_cfg

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)


def make_level(batch, shape, n, seed, order="sorted"):
    """n distinct sites (b, z, y, x) of a [batch, *shape] lattice, int32 on the GPU, in canonical order or shuffled."""
    g = torch.Generator().manual_seed(seed)
    total = batch * shape[0] * shape[1] * shape[2]
    lin = torch.randperm(total, generator=g)[:n]
    if order == "sorted":
        lin = lin.sort().values
    z_y_x = shape[0] * shape[1] * shape[2]
    b = lin // z_y_x
    r = lin % z_y_x
    coords = torch.stack([b, r // (shape[1] * shape[2]), (r // shape[2]) % shape[1], r % shape[2]], dim=1)
    return coords.int().to(DEV)


def grid_points(batch, m, lo, hi, seed):
    """m points per sample uniformly in [lo, hi) (beyond the lattice on every side), sample index in the column order of the
    reference's roi_grid_pool (all points of sample 0, then sample 1, ...)."""
    g = torch.Generator().manual_seed(seed)
    lo, hi = torch.tensor(lo), torch.tensor(hi)
    xyz = (torch.rand((batch * m, 3), generator=g) * (hi - lo) + lo).float().to(DEV)
    bidx = torch.arange(batch).repeat_interleave(m).float().view(-1, 1).to(DEV)
    return xyz, bidx


def coords_of(xyz, bidx, pc_range, voxel_size, stride):
    """The reference's grid coordinates: torch // of floats per axis, // stride, [b, x, y, z] -> int -> (b, z, y, x)."""
    c = torch.cat([(xyz[:, j:j + 1] - pc_range[j]) // voxel_size[j] for j in range(3)], dim=1)
    c = torch.cat([bidx, c // stride], dim=1).int()
    return c[:, [0, 3, 2, 1]].contiguous()


PC_RANGE = [0.0, -8.0, -2.0, 12.8, 8.0, 2.0]
VSIZE = [0.1, 0.1, 0.2]


def query_case(batch, shape, n, m, stride, radius, rng, nsample, seed, gi_kind):
    order = "sorted" if gi_kind != "unordered" else "shuffled"
    coords = make_level(batch, shape, n, seed, order)
    xyz = get_voxel_centers(coords[:, 1:4], stride, VSIZE, PC_RANGE).contiguous()
    lo = [PC_RANGE[j] - 1.0 for j in range(3)]
    hi = [PC_RANGE[3 + j] + 1.0 for j in range(3)]
    new_xyz, bidx = grid_points(batch, m, lo, hi, seed + 1)
    new_coords = coords_of(new_xyz, bidx, PC_RANGE, VSIZE, stride)
    if gi_kind == "unordered":
        gi = ops.GridIndex.from_coords_unordered(coords, batch, shape)
    else:
        gi = ops.GridIndex.from_coords(coords, batch, shape)
        if gi_kind == "canonical":
            gi.rowof = None        # sorted sites: ranks are the rows (the strided-conv levels)
    level = VoxelLevel(coords, list(shape), batch, gi)
    got = ops.voxel_query(new_xyz, new_coords, xyz, gi, radius, rng, nsample)
    want = voxel_query_torch(new_xyz, new_coords, xyz, level, radius, rng, nsample)
    return got, want, new_coords


@pytest.mark.parametrize("gi_kind", ["canonical", "rowof", "unordered"])
def test_voxel_query_matches_torch_restatement_on_a_hand_built_level(gi_kind):
    shape = [10, 80, 64]          # stride 2 over the 0.1 x 0.1 x 0.2 grid of PC_RANGE
    for radius, nsample, n, rng in ((0.45, 16, 6000, (2, 3, 3)), (1.5, 4, 20000, (2, 2, 2)), (0.05, 8, 3000, (1, 1, 1))):
        (idx, empty), (idx_t, empty_t), nc = query_case(2, shape, n, 3000, 2, radius, rng, nsample, 7, gi_kind)
        assert torch.equal(idx, idx_t) and torch.equal(empty, empty_t), (radius, nsample)
        e = empty.cpu()
        off = ((nc[:, 1] < 0) | (nc[:, 1] >= shape[0]) | (nc[:, 2] < 0) | (nc[:, 2] >= shape[1]) | (nc[:, 3] < 0) | (nc[:, 3] >= shape[2])).cpu()
        assert off.any()                                     # grid points off the lattice
        assert e.any() and (~e).any()                       # empty and non-empty balls
        if nsample == 4:                                     # saturated balls: four distinct rows
            full = (idx[:, 1:] != idx[:, :1]).all(dim=1)
            assert bool(full.any())
        b = nc[:, 0].cpu()
        assert bool((~e[b == 0]).any()) and bool((~e[b == 1]).any())     # both batch ends hit


def test_voxel_query_at_waymo_training_shape():
    # x_conv2 of the Waymo grid (41 x 1504 x 1504 at 0.1 x 0.1 x 0.15 -> stride 2), bs 4 x 128 rois x 6^3 grid points
    pc = [-75.2, -75.2, -2.0, 75.2, 75.2, 4.0]
    vs = [0.1, 0.1, 0.15]
    shape = [21, 752, 752]
    g = torch.Generator().manual_seed(3)
    coords = []
    for b in range(4):                                               # a dense cluster of sites around the origin per sample
        z = torch.randint(0, shape[0], (60000,), generator=g)
        y = torch.randint(300, 452, (60000,), generator=g)
        x = torch.randint(300, 452, (60000,), generator=g)
        coords.append(torch.stack([torch.full_like(z, b), z, y, x], 1))
    coords = torch.unique(torch.cat(coords), dim=0).int().to(DEV)
    xyz = get_voxel_centers(coords[:, 1:4], 2, vs, pc).contiguous()
    m = 128 * 216
    new_xyz = (torch.rand((4 * m, 3), generator=g) * torch.tensor([20.0, 20.0, 5.0]) - torch.tensor([10.0, 10.0, 2.0])).float().to(DEV)
    bidx = torch.arange(4).repeat_interleave(m).float().view(-1, 1).to(DEV)
    nc = coords_of(new_xyz, bidx, pc, vs, 2)
    gi = ops.GridIndex.from_coords(coords, 4, shape)
    gi.rowof = None
    level = VoxelLevel(coords, shape, 4, gi)
    idx, empty = ops.voxel_query(new_xyz, nc, xyz, gi, 0.4, (3, 3, 2), 16)
    idx_t, empty_t = voxel_query_torch(new_xyz, nc, xyz, level, 0.4, (3, 3, 2), 16)
    assert torch.equal(idx, idx_t) and torch.equal(empty, empty_t)
    assert bool((~empty).any()) and bool(empty.any())


def pool_inputs(seed, n=4000, m=2500, c=32, nsample=16, gamma_pos=0.02, spacing=0.5, radius=0.6):
    """A level, its query and features whose pooled maxima beat every other voxel's value by far more than fp32 rounding:
    per channel the rows carry distinct multiples of `spacing` (+ spacing / 2), while the position term (BatchNorm2d scale
    gamma_pos, so about 4 gamma_pos at most) varies by well under spacing / 2."""
    shape = [10, 80, 64]
    (idx, empty), _, _ = query_case(2, shape, n, m // 2, 2, radius, (2, 3, 3), nsample, seed, "rowof")
    coords = make_level(2, shape, n, seed, "sorted")
    xyz = get_voxel_centers(coords[:, 1:4], 2, VSIZE, PC_RANGE).contiguous()
    lo = [PC_RANGE[j] - 1.0 for j in range(3)]
    hi = [PC_RANGE[3 + j] + 1.0 for j in range(3)]
    new_xyz, _ = grid_points(2, m // 2, lo, hi, seed + 1)
    g = torch.Generator().manual_seed(seed + 2)
    f = (torch.stack([torch.randperm(n, generator=g) for _ in range(c)], dim=1).float() + 0.5 - 0.5 * n) * spacing
    torch.manual_seed(seed)
    pos = torch.nn.Sequential(torch.nn.Conv2d(3, c, 1, bias=False), torch.nn.BatchNorm2d(c))
    with torch.no_grad():
        pos[1].weight.uniform_(0.5 * gamma_pos, gamma_pos)
        pos[1].bias.uniform_(0.5 * gamma_pos, gamma_pos)
        pos[1].bias.mul_(torch.randint(0, 2, (c,)).float() * 2 - 1)       # |b| >= gamma_pos / 2: empty balls keep a clear sign
    return f.to(DEV), idx, empty, xyz, new_xyz, pos.to(DEV)


def ref64(f, idx, empty, xyz, new_xyz, pos):
    p64 = copy.deepcopy(pos).double()
    f64 = f.detach().double().requires_grad_(True)
    out = pool_torch(f64, idx, empty, xyz.double(), new_xyz.double(), p64)
    return out, f64, p64


def assert_margin(f, idx, empty, xyz, new_xyz, pos):
    """In fp64: every positive pooled maximum exceeds the best value from another voxel by > 0.05, and no maximum lies within
    0.005 of 0 (the ReLU's kink)."""
    with torch.no_grad():
        p64 = copy.deepcopy(pos).double()
        rows = idx.long()
        gf = f.double()[rows]                                          # (M, ns, C)
        gf[empty] = 0
        d = xyz.double()[rows] - new_xyz.double().unsqueeze(1)
        d[empty] = 0
        v = gf + p64(d.permute(2, 0, 1).unsqueeze(0)).squeeze(0).permute(1, 2, 0)
        best, at = v.max(dim=1)
        other = torch.where(rows.unsqueeze(-1) == rows.gather(1, at).unsqueeze(1), torch.full_like(v, -1e30), v).max(dim=1).values
        pos_max = best > 0
        assert bool(((best - other)[pos_max] > 0.05).all())
        assert bool((best.abs() > 0.005).all())


def bound(got, want64, torch32):
    ref = want64.detach()
    err = float((got.detach().double() - ref).abs().max())
    err_t = float((torch32.detach().double() - ref).abs().max())
    return err, max(2.0 * err_t, 1e-5 * float(ref.abs().max()))


@pytest.mark.parametrize("training", [True, False])
def test_pool_forward_matches_fp64_composition(training):
    f, idx, empty, xyz, new_xyz, pos = pool_inputs(11)
    if not training:
        with torch.no_grad():
            pos[1].running_mean.uniform_(-0.1, 0.1)
            pos[1].running_var.uniform_(0.5, 2.0)
    pos.train(training)
    pos_t = copy.deepcopy(pos)
    want, _, p64 = ref64(f, idx, empty, xyz, new_xyz, pos)
    t32 = pool_torch(f, idx, empty, xyz, new_xyz, pos_t)
    a, b = folded_position_map(pos, idx, empty, xyz, new_xyz)
    got = ops.voxel_neighbor_pool(f, a, b, idx, empty, xyz, new_xyz)
    err, tol = bound(got, want, t32)
    assert err <= tol, (err, tol)
    for name in ("running_mean", "running_var"):
        assert torch.allclose(getattr(pos[1], name), getattr(pos_t[1], name), rtol=1e-5, atol=1e-6), name
    assert int(pos[1].num_batches_tracked) == int(pos_t[1].num_batches_tracked)


def test_pool_backward_matches_fp64_composition():
    f, idx, empty, xyz, new_xyz, pos = pool_inputs(13)
    assert_margin(f, idx, empty, xyz, new_xyz, pos)
    pos_t = copy.deepcopy(pos)
    gout = torch.randn((idx.shape[0], f.shape[1]), generator=torch.Generator().manual_seed(5)).to(DEV)
    want, f64, p64 = ref64(f, idx, empty, xyz, new_xyz, pos)
    want.backward(gout.double())
    ft = f.clone().requires_grad_(True)
    pool_torch(ft, idx, empty, xyz, new_xyz, pos_t).backward(gout)
    fk = f.clone().requires_grad_(True)
    a, b = folded_position_map(pos, idx, empty, xyz, new_xyz)
    ops.voxel_neighbor_pool(fk, a, b, idx, empty, xyz, new_xyz).backward(gout)
    pairs = [(fk.grad, f64.grad, ft.grad)]
    for pk, p6, pt in zip(pos.parameters(), p64.parameters(), pos_t.parameters()):
        pairs.append((pk.grad, p6.grad, pt.grad))
    for k, (g_k, g_64, g_t) in enumerate(pairs):
        err, tol = bound(g_k, g_64, g_t)
        assert err <= tol, (k, err, tol)


def test_module_forward_backward_matches_fp64_and_is_reproducible(monkeypatch):
    """NeighborVoxelSAModuleMSG on the GPU (row matmuls + bn_rows + the fused pool) against its plain-torch CPU path in fp64:
    output and the gradients of the features and of every mlps_in / mlps_pos / mlps_out parameter; two runs bit-identical.
    The fp32 yardstick is the same module on the GPU with the reference's torch composition in place of the fused pool, so
    mlps_in and mlps_out run through the same matmuls in the same reduction order in both and the bound measures the pool."""
    from toda_amd.pcdet.ops.pointnet2.pointnet2_stack import voxel_pool_modules as vpm

    f, idx, empty, xyz, new_xyz, pos = pool_inputs(17, n=1500, c=32, spacing=0.25)
    assert_margin(f, idx, empty, xyz, new_xyz, pos)
    n, c = f.shape
    coords = make_level(2, [10, 80, 64], n, 17, "sorted")
    bidx = torch.arange(2).repeat_interleave(idx.shape[0] // 2).float().view(-1, 1).to(DEV)
    ref_coords = torch.cat([bidx, torch.cat([(new_xyz[:, j:j + 1] - PC_RANGE[j]) // VSIZE[j] for j in range(3)], 1) // 2], 1).int()
    torch.manual_seed(0)
    mod = NeighborVoxelSAModuleMSG(query_ranges=[[2, 3, 3]], radii=[0.6], nsamples=[16], mlps=[[c, c, 16]]).to(DEV).train()
    with torch.no_grad():
        mod.mlps_in[0][0].weight.copy_(torch.eye(c).unsqueeze(-1))               # identity + BN scaled back: spacing of f kept
        mod.mlps_in[0][1].weight.copy_(f.std(dim=0, unbiased=False))
        mod.mlps_pos[0].load_state_dict(pos.state_dict())
    mod64 = copy.deepcopy(mod).double().cpu()
    snap = copy.deepcopy(mod.state_dict())
    gout = torch.randn((idx.shape[0], 16), generator=torch.Generator().manual_seed(9))

    def run_gpu():
        mod.load_state_dict(snap)
        mod.zero_grad()
        fg = f.clone().requires_grad_(True)
        out = mod(xyz, None, new_xyz, None, ref_coords, fg, VoxelLevel(coords, [10, 80, 64], 2))
        out.backward(gout.to(DEV))
        return out.detach(), fg.grad, [p.grad.clone() for p in mod.parameters()]

    o1, g1, p1 = run_gpu()
    o2, g2, p2 = run_gpu()
    assert torch.equal(o1, o2) and torch.equal(g1, g2) and all(torch.equal(a, b) for a, b in zip(p1, p2))

    with monkeypatch.context() as mp:       # the fp32 torch composition on the GPU: mlps_pos as modules, grouped tensors, max_pool2d
        mp.setattr(vpm, "folded_position_map", lambda mlp_pos, *a: (mlp_pos, None))
        mp.setattr(ops, "voxel_neighbor_pool", lambda fin, mlp_pos, _, i, e, x, nx: pool_torch(fin, i, e, x, nx, mlp_pos))
        o32, g32, p32 = run_gpu()

    f64 = f.detach().double().cpu().requires_grad_(True)
    out64 = mod64(xyz.double().cpu(), None, new_xyz.double().cpu(), None, ref_coords.cpu(), f64, VoxelLevel(coords.cpu(), [10, 80, 64], 2))
    out64.backward(gout.double())
    err, tol = bound(o1.cpu(), out64, o32.cpu())
    assert err <= tol, ("out", err, tol)
    err, tol = bound(g1.cpu(), f64.grad, g32.cpu())
    assert err <= tol, ("features", err, tol)
    for (name, _), gk, p6, p3 in zip(mod.named_parameters(), p1, mod64.parameters(), p32):
        err, tol = bound(gk.cpu(), p6.grad, p3.cpu())
        assert err <= tol, (name, err, tol)


@pytest.mark.parametrize("training", [True, False])
def test_pool_forward_position_term_alone(training):
    """f = 0: the pooled value is max_s relu(mlps_pos(d)), so the folded map a . d + b carries the whole result (train: batch
    statistics W mu / W^T Sigma W; eval: running statistics), with unit-scale BatchNorm2d parameters."""
    f, idx, empty, xyz, new_xyz, pos = pool_inputs(23, gamma_pos=1.0)
    f = torch.zeros_like(f)
    with torch.no_grad():
        pos[1].running_mean.uniform_(-0.2, 0.2)
        pos[1].running_var.uniform_(0.05, 0.5)
    pos.train(training)
    pos_t = copy.deepcopy(pos)
    want, _, _ = ref64(f, idx, empty, xyz, new_xyz, pos)
    t32 = pool_torch(f, idx, empty, xyz, new_xyz, pos_t)
    a, b = folded_position_map(pos, idx, empty, xyz, new_xyz)
    got = ops.voxel_neighbor_pool(f, a, b, idx, empty, xyz, new_xyz)
    assert float(want.abs().max()) > 0.5 and float((want > 0).float().mean()) > 0.3
    err, tol = bound(got, want, t32)
    assert err <= tol, (err, tol)


def test_pool_kernels_are_reproducible_and_use_integer_atomics_only():
    import os
    import re

    f, idx, empty, xyz, new_xyz, pos = pool_inputs(19, n=6000, m=4000, c=64)
    gout = torch.randn((idx.shape[0], 64), device=DEV)
    snap = copy.deepcopy(pos.state_dict())
    res = []
    for _ in range(2):
        pos.load_state_dict(snap)
        pos.zero_grad()
        fk = f.clone().requires_grad_(True)
        a, b = folded_position_map(pos, idx, empty, xyz, new_xyz)
        out = ops.voxel_neighbor_pool(fk, a, b, idx, empty, xyz, new_xyz)
        out.backward(gout)
        res.append([out.detach(), fk.grad] + [p.grad.clone() for p in pos.parameters()] + [pos[1].running_var.clone()])
    assert all(torch.equal(x, y) for x, y in zip(*res))
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "toda_amd", "csrc", "voxel_pool.hip")).read()
    # the only atomic add of the file counts entries per row (int32); no float accumulator is ever an atomic target
    assert "unsafeAtomicAdd" not in src
    assert set(re.findall(r"atomicAdd\s*\(\s*&?\s*(\w+)", src)) == {"cnt"}
    assert re.search(r"int32_t\* __restrict__ cnt\)", src)


def _small(cfg):
    cfg.DATA_CONFIG.SYNTHETIC.NUM_POINTS = 12000
    return cfg


def test_voxel_rcnn_kitti_trains_three_steps_and_evaluates():
    from toda_amd.pcdet.datasets import SyntheticLidarDataset
    from toda_amd.pcdet.models import build_network, load_data_to_gpu, prepare_batch_on_gpu

    cfg = _small(load_cfg("voxel_rcnn_kitti"))
    ds = SyntheticLidarDataset(cfg.DATA_CONFIG, cfg.CLASS_NAMES, training=True)
    torch.manual_seed(0)
    np.random.seed(0)
    net = build_network(cfg.MODEL, len(cfg.CLASS_NAMES), ds).cuda().train()
    opt = torch.optim.Adam(net.parameters(), lr=1e-3)
    for step in range(3):
        batch = ds.collate_batch([ds[2 * step], ds[2 * step + 1]])
        prepare_batch_on_gpu(batch, net)
        opt.zero_grad()
        ret, tb, _ = net(batch)
        loss = ret["loss"]
        assert torch.isfinite(loss), (step, tb)
        for k in ("loss_rpn", "rcnn_loss_cls", "rcnn_loss_reg", "rcnn_loss"):
            assert torch.isfinite(torch.as_tensor(tb[k])), k
        loss.backward()
        grads = [p.grad for p in net.roi_head.roi_grid_pool_layers.parameters() if p.grad is not None]
        assert grads and all(torch.isfinite(gr).all() for gr in grads)
        assert float(sum(gr.abs().sum() for gr in grads)) > 0
        bb = [p.grad for p in net.backbone_3d.conv2.parameters() if p.grad is not None]
        assert bb and float(sum(gr.abs().sum() for gr in bb)) > 0          # the pool trains x_conv2 end to end
        opt.step()
    net.eval()
    test_ds = SyntheticLidarDataset(cfg.DATA_CONFIG, cfg.CLASS_NAMES, training=False)
    batch = test_ds.collate_batch([test_ds[0], test_ds[1]])
    load_data_to_gpu(batch)
    prepare_batch_on_gpu(batch, net)
    with torch.no_grad():
        preds, recall = net(batch)
    assert len(preds) == 2
    for p in preds:
        n = p["pred_boxes"].shape[0]
        assert p["pred_scores"].shape[0] == n and p["pred_labels"].shape[0] == n
    assert recall["gt"] > 0
    for t in cfg.MODEL.POST_PROCESSING.RECALL_THRESH_LIST:
        assert f"roi_{t}" in recall and f"rcnn_{t}" in recall


def test_voxel_rcnn_waymo_trains_through_input_prefetcher_and_evaluates():
    from toda_amd.pcdet.datasets import SyntheticLidarDataset
    from toda_amd.pcdet.models import InputPrefetcher, build_network, load_data_to_gpu, prepare_batch_on_gpu

    cfg = load_cfg("voxel_rcnn_dyn_voxel_waymo")
    cfg.DATA_CONFIG.SYNTHETIC.NUM_POINTS = 40000
    ds = SyntheticLidarDataset(cfg.DATA_CONFIG, cfg.CLASS_NAMES, training=True)
    torch.manual_seed(0)
    np.random.seed(0)
    net = build_network(cfg.MODEL, len(cfg.CLASS_NAMES), ds).cuda().train()
    pre = InputPrefetcher(iter([ds.collate_batch([ds[0], ds[1]])]), net, torch.device("cuda", 0))
    try:
        batch = pre.next()
        ret, tb, _ = net(batch)
        loss = ret["loss"]
        loss.backward()
    finally:
        pre.close()
    assert torch.isfinite(loss), tb
    for k in ("rcnn_loss_cls", "rcnn_loss_reg", "rcnn_loss"):
        assert torch.isfinite(torch.as_tensor(tb[k])), k
    assert float(sum(p.grad.abs().sum() for p in net.roi_head.parameters() if p.grad is not None)) > 0
    net.eval()
    test_ds = SyntheticLidarDataset(cfg.DATA_CONFIG, cfg.CLASS_NAMES, training=False)
    batch = test_ds.collate_batch([test_ds[0], test_ds[1]])
    load_data_to_gpu(batch)
    prepare_batch_on_gpu(batch, net)
    with torch.no_grad():
        preds, recall = net(batch)
    assert len(preds) == 2
    for t in cfg.MODEL.POST_PROCESSING.RECALL_THRESH_LIST:
        assert f"roi_{t}" in recall and f"rcnn_{t}" in recall


def test_head_matches_reference_fixture_on_the_gpu():
    """VoxelRCNNHead on the GPU (HIP query, fused pool, row matmuls, device IoU in the sampler) against the reference fixture:
    eval predictions, the sampled rois and labels, the loss terms, and the gradients of every parameter and of both levels."""
    from tests.test_voxel_rcnn_host import check_head_against_fixture

    check_head_against_fixture("cuda", rtol=1e-4, atol=1e-5, grad_rtol=1e-4)
