"""PV-RCNN on the MI355X: FPS and the stacked ball query against torch restatements of the reference's kernels (exact, index for
index), the SA pool forward and backward and the BEV interpolation against fp64 evaluations of the reference's compositions,
BatchNorm2d running statistics, run-to-run reproducibility, and both configurations training and evaluating."""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from toda_amd import ops
from toda_amd.pcdet.models.backbones_3d.pfe.voxel_set_abstraction import bilinear_interpolate_torch
from toda_amd.pcdet.ops.pointnet2.pointnet2_stack import pointnet2_utils
from toda_amd.pcdet.ops.pointnet2.pointnet2_stack.pointnet2_modules import StackSAModuleMSG

from tests.test_pv_rcnn_host import load_cfg

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)


def cloud(n, seed, extent=(70.0, 70.0, 4.0), dup=0):
    g = torch.Generator().manual_seed(seed)
    p = (torch.rand((n, 3), generator=g) - 0.5) * torch.tensor(extent)
    p = (p * 8).round() / 8                                   # a coarse lattice: exact distance ties
    if dup:
        p[-dup:] = p[:dup]                                     # duplicated points
    return p.float()


def fps_restated(xyz, npoint):
    return pointnet2_utils.fps_torch(xyz.to(DEV), npoint).cpu()


@pytest.mark.parametrize("n,npoint,dup", [(20000, 2048, 0), (1500, 512, 300), (1024, 256, 100), (700, 1024, 50)])
def test_fps_matches_the_reference_kernel_index_for_index(n, npoint, dup):
    xyz = cloud(n, n, dup=dup)
    want = fps_restated(xyz, npoint)
    for mode in (1, 2):
        got = ops.farthest_point_sample(xyz.to(DEV), [n], npoint, mode=mode).cpu().long()[0]
        if n >= npoint:
            assert torch.equal(got, want), (mode, int((got != want).nonzero()[0]))
        else:                                                # VoxelSetAbstraction keeps the first N picks
            assert torch.equal(got[:n], want[:n]), mode


def test_fps_at_the_waymo_shape_both_samples_in_one_launch():
    counts = [180000, 171000]
    xyz = torch.cat([cloud(counts[0], 1), cloud(counts[1], 2)], 0)
    got = ops.farthest_point_sample(xyz.to(DEV), counts, 4096, mode=2).cpu().long()
    ops.L.check(ops.L.load().toda_device_fault(), "toda_device_fault")
    assert torch.equal(got[0], fps_restated(xyz[:counts[0]], 4096))
    assert torch.equal(got[1], fps_restated(xyz[counts[0]:], 4096))
    auto = ops.farthest_point_sample(xyz.to(DEV), counts, 4096).cpu().long()
    assert torch.equal(auto, got)


def ball_query_restated(radius, nsample, xyz, xs, new_xyz, ns_):
    """Vectorised restatement of ball_query_gpu.cu on the GPU: rows of xyz, zeros and the flag for an empty ball."""
    m = new_xyz.shape[0]
    idx = torch.zeros((m, nsample), dtype=torch.int64, device=DEV)
    empty = torch.zeros((m,), dtype=torch.bool, device=DEV)
    r2 = torch.tensor(radius, dtype=torch.float32) * torch.tensor(radius, dtype=torch.float32)
    for b in range(len(xs) - 1):
        pts = xyz[xs[b]:xs[b + 1]]
        if pts.shape[0] == 0:                                 # a sample without points: every ball of its queries is empty
            empty[ns_[b]:ns_[b + 1]] = True
            continue
        for q0 in range(ns_[b], ns_[b + 1], 512):
            q1 = min(q0 + 512, ns_[b + 1])
            c = new_xyz[q0:q1]
            d2 = (c[:, 0:1] - pts[None, :, 0]) * (c[:, 0:1] - pts[None, :, 0]) + (c[:, 1:2] - pts[None, :, 1]) * (c[:, 1:2] - pts[None, :, 1]) \
                + (c[:, 2:3] - pts[None, :, 2]) * (c[:, 2:3] - pts[None, :, 2])
            hit = d2 < r2.to(DEV)
            pos = torch.cumsum(hit.int(), 1) - 1
            take = hit & (pos < nsample)
            cnt = hit.sum(1)
            first = torch.argmax(hit.int(), 1)
            blk = (first + xs[b]).unsqueeze(1).repeat(1, nsample)
            r, k = take.nonzero(as_tuple=True)
            blk[r, pos[r, k]] = k + xs[b]
            blk[cnt == 0] = 0
            idx[q0:q1] = blk
            empty[q0:q1] = cnt == 0
    return idx.int(), empty


@pytest.mark.parametrize("shape", ["vsa", "roi_grid"])
def test_ball_query_matches_its_restatement_exactly(shape):
    if shape == "vsa":     # Waymo x_conv3-like voxel centres around 2 x 4096 keypoints, radii 1.2 / 2.4, nsample 16 / 32
        counts, m_per, radii, nsamples = [30000, 26000], 4096, [1.2, 2.4], [16, 32]
    else:                  # keypoints around the 2 x 128 x 216 RoI grid points, radii 0.8 / 1.6, nsample 16 / 16
        counts, m_per, radii, nsamples = [4096, 4096], 128 * 216, [0.8, 1.6], [16, 16]
    xyz = torch.cat([cloud(c, 10 + i, extent=(40.0, 40.0, 4.0)) for i, c in enumerate(counts)], 0).to(DEV)
    new_xyz = torch.cat([cloud(m_per, 20 + i, extent=(44.0, 44.0, 5.0)) for i in range(2)], 0).to(DEV)
    xs = [0, counts[0], counts[0] + counts[1]]
    ns_ = [0, m_per, 2 * m_per]
    got = ops.ball_query_stack(radii, nsamples, xyz, ops.batch_starts(counts, DEV), new_xyz, ops.batch_starts([m_per, m_per], DEV))
    for (idx, empty), r, ns in zip(got, radii, nsamples):
        want_idx, want_empty = ball_query_restated(r, ns, xyz, xs, new_xyz, ns_)
        assert torch.equal(empty, want_empty)
        assert torch.equal(idx, want_idx)
        assert 0 < int(empty.sum()) < empty.numel() or shape == "vsa"
    again = ops.ball_query_stack(radii, nsamples, xyz, ops.batch_starts(counts, DEV), new_xyz, ops.batch_starts([m_per, m_per], DEV))
    assert all(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) for a, b in zip(got, again))


def _sa_setup(c_in=13, mlps=((32, 32), (32,)), radii=(0.8, 1.6), nsamples=(16, 32), seed=0):
    torch.manual_seed(seed)
    mod = StackSAModuleMSG(radii=list(radii), nsamples=list(nsamples), mlps=[[c_in] + list(m) for m in mlps])
    for p in mod.parameters():
        with torch.no_grad():
            p.add_(torch.randn_like(p) * 0.1)
    counts, m_per = [900, 700], [300, 200]
    xyz = torch.cat([cloud(c, 40 + i, extent=(12.0, 12.0, 3.0)) for i, c in enumerate(counts)], 0)
    new_xyz = torch.cat([cloud(m, 50 + i, extent=(14.0, 14.0, 3.5)) for i, m in enumerate(m_per)], 0)
    feats = torch.randn((xyz.shape[0], c_in), generator=torch.Generator().manual_seed(seed + 1))
    return mod, counts, m_per, xyz, new_xyz, feats


def test_sa_pool_forward_backward_match_fp64_composition():
    mod, counts, m_per, xyz, new_xyz, feats = _sa_setup()
    ref = copy.deepcopy(mod).double().train()
    gpu = mod.to(DEV).train()
    f_gpu = feats.to(DEV).requires_grad_(True)
    _, out = gpu(xyz.to(DEV), counts, new_xyz.to(DEV), m_per, f_gpu)
    gout = torch.randn(out.shape, generator=torch.Generator().manual_seed(7))
    out.backward(gout.to(DEV))

    # fp64 reference composition on the tables the kernel found (the query itself is checked exactly above)
    tables = pointnet2_utils.ball_query_multi(gpu.radii, gpu.nsamples, xyz.to(DEV), counts, new_xyz.to(DEV), m_per)
    f64 = feats.double().requires_grad_(True)
    outs = []
    for k, (idx, empty) in enumerate(tables):
        grouped = pointnet2_utils.QueryAndGroup.group(xyz.double(), new_xyz.double(), f64, idx.cpu(), empty.cpu(), True)
        y = ref.mlps[k](grouped.permute(1, 0, 2).unsqueeze(0))
        outs.append(F.max_pool2d(y, kernel_size=[1, y.size(3)]).squeeze(-1).squeeze(0).permute(1, 0))
    want = torch.cat(outs, 1)
    want.backward(gout.double())
    scale = float(want.detach().abs().max())
    assert float((out.detach().cpu().double() - want.detach()).abs().max()) < 2e-5 * scale
    gs = float(f64.grad.abs().max())
    assert float((f_gpu.grad.cpu().double() - f64.grad).abs().max()) < 1e-4 * gs
    for (name, p), (_, q) in zip(gpu.named_parameters(), ref.named_parameters()):
        assert float((p.grad.cpu().double() - q.grad).abs().max()) < 1e-4 * max(float(q.grad.abs().max()), 1e-6), name
    for (name, b), (_, c) in zip(gpu.named_buffers(), ref.named_buffers()):
        assert float((b.cpu().double() - c.double()).abs().max()) < 1e-4 * max(float(c.double().abs().max()), 1.0), name


def test_sa_pool_eval_matches_and_is_reproducible():
    mod, counts, m_per, xyz, new_xyz, feats = _sa_setup(seed=3)
    ref = copy.deepcopy(mod).double().eval()
    gpu = mod.to(DEV).eval()
    with torch.no_grad():
        _, a = gpu(xyz.to(DEV), counts, new_xyz.to(DEV), m_per, feats.to(DEV))
        _, b = gpu(xyz.to(DEV), counts, new_xyz.to(DEV), m_per, feats.to(DEV))
        _, want = ref(xyz.double(), counts, new_xyz.double(), m_per, feats.double())
    assert torch.equal(a, b)
    assert float((a.cpu().double() - want).abs().max()) < 2e-5 * float(want.abs().max())


def test_sa_kernels_backward_are_bitwise_reproducible():
    mod, counts, m_per, xyz, new_xyz, feats = _sa_setup(seed=5)
    gpu = mod.to(DEV).train()
    grads = []
    for _ in range(2):
        f = feats.to(DEV).requires_grad_(True)
        gpu.zero_grad()
        _, out = gpu(xyz.to(DEV), counts, new_xyz.to(DEV), m_per, f)
        out.square().sum().backward()
        grads.append([f.grad.clone()] + [p.grad.clone() for p in gpu.parameters()])
    assert all(torch.equal(a, b) for a, b in zip(*grads))


def test_bev_interpolation_forward_backward_match_fp64():
    g = torch.Generator().manual_seed(0)
    fmap = torch.randn((2, 24, 47, 53), generator=g)
    k = 3000
    x = torch.rand((k,), generator=g) * 58 - 2.5                # taps beyond the map on every side: clamped
    y = torch.rand((k,), generator=g) * 52 - 2.5
    bidx = (torch.arange(k) >= k // 2).int()
    fm = fmap.to(DEV).requires_grad_(True)
    out = ops.bev_interpolate(fm, x.to(DEV), y.to(DEV), bidx.to(DEV))
    gout = torch.randn(out.shape, generator=g)
    out.backward(gout.to(DEV))
    f64 = fmap.double().requires_grad_(True)
    want = torch.cat([bilinear_interpolate_torch(f64[b].permute(1, 2, 0), x[bidx == b].double(), y[bidx == b].double()) for b in range(2)])
    want.backward(gout.double())
    assert float((out.detach().cpu().double() - want).abs().max()) < 1e-5 * float(want.abs().max())
    assert float((fm.grad.cpu().double() - f64.grad).abs().max()) < 1e-5 * float(f64.grad.abs().max())
    # fp32 torch on the same map: the kernel restates its formulas and sum order
    want32 = torch.cat([bilinear_interpolate_torch(fmap[b].permute(1, 2, 0), x[bidx == b], y[bidx == b]) for b in range(2)])
    assert torch.equal(out.detach().cpu(), want32)
    fm2 = fmap.to(DEV).requires_grad_(True)
    ops.bev_interpolate(fm2, x.to(DEV), y.to(DEV), bidx.to(DEV)).backward(gout.to(DEV))
    assert torch.equal(fm2.grad, fm.grad)


def _train_and_eval(name, prefetch):
    from toda_amd.pcdet.datasets import SyntheticLidarDataset
    from toda_amd.pcdet.models import InputPrefetcher, build_network, load_data_to_gpu, prepare_batch_on_gpu

    cfg = load_cfg(name)
    cfg.DATA_CONFIG.SYNTHETIC.NUM_POINTS = 30000
    ds = SyntheticLidarDataset(cfg.DATA_CONFIG, cfg.CLASS_NAMES, training=True)
    torch.manual_seed(0)
    np.random.seed(0)
    net = build_network(cfg.MODEL, len(cfg.CLASS_NAMES), ds).cuda().train()
    opt = torch.optim.Adam(net.parameters(), lr=1e-3)
    for step in range(3):
        raw = ds.collate_batch([ds[2 * step], ds[2 * step + 1]])
        if prefetch:
            pre = InputPrefetcher(iter([raw]), net, DEV)
            try:
                batch = pre.next()
            finally:
                pre.close()
        else:
            batch = raw
            prepare_batch_on_gpu(batch, net)
        opt.zero_grad()
        ret, tb, _ = net(batch)
        loss = ret["loss"]
        assert torch.isfinite(loss), (step, tb)
        for k in ("loss_rpn", "point_loss_cls", "rcnn_loss_cls", "rcnn_loss_reg", "rcnn_loss"):
            assert torch.isfinite(torch.as_tensor(tb[k])), k
        loss.backward()
        for part in (net.pfe, net.point_head, net.roi_head.roi_grid_pool_layer):
            grads = [p.grad for p in part.parameters() if p.grad is not None]
            assert grads and all(torch.isfinite(gr).all() for gr in grads)
            assert float(sum(gr.abs().sum() for gr in grads)) > 0
        opt.step()
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
    ops.L.check(ops.L.load().toda_device_fault(), "toda_device_fault")


def test_pv_rcnn_kitti_trains_three_steps_and_evaluates():
    _train_and_eval("pv_rcnn_kitti", prefetch=False)


def test_pv_rcnn_waymo_trains_through_input_prefetcher_and_evaluates():
    _train_and_eval("pv_rcnn_centerhead_waymo", prefetch=True)


def test_fps_and_ball_query_match_reference_fixtures_on_the_gpu():
    from tests.test_pv_rcnn_fixtures import check_ball_query, check_fps

    check_fps("cuda")
    check_ball_query("cuda")


def test_vsa_and_point_head_match_reference_fixtures_on_the_gpu():
    from tests.test_pv_rcnn_fixtures import check_point_head, check_vsa

    check_vsa("cuda", rtol=1e-4, atol=1e-4)
    check_point_head("cuda", rtol=1e-4, atol=1e-4)


def test_pvrcnn_head_matches_reference_fixture_on_the_gpu():
    """PVRCNNHead on the GPU (HIP ball query, SA pool, row matmuls, device IoU in the sampler): eval predictions, the sampled rois
    and labels, the loss terms, and the gradients of every parameter and of the keypoint features."""
    from tests.test_pv_rcnn_fixtures import check_pv_head

    check_pv_head("cuda", rtol=1e-4, atol=1e-5, grad_rtol=1e-4)
