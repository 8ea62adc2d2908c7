"""SECOND-IoU on the MI355X (csrc/roi_head.hip through the C ABI): the grid pool matches the reference fixture and torch's
affine_grid / grid_sample at the TODA shape and is bit-reproducible; the 3-D IoU max matches the oracle; the proposal targets,
the head's forward / loss / gradients match the reference fixtures; both SECOND-IoU configurations train and evaluate."""
import os

import numpy as np
import pytest
import torch

from oracle import oracle as O
from toda_amd import ops
from toda_amd.pcdet.models.roi_heads.second_head import roi_grid_pool_torch

from tests.test_second_iou_host import GOLDEN, TARGET_CONFIG, head_cfg, load_cfg

pytestmark = pytest.mark.gpu


def small_dataset_cfg():
    from toda_amd.pcdet.config import AttrDict

    return AttrDict(dict(POINT_CLOUD_RANGE=[-4.0, -5.0, -3.0, 6.0, 5.0, 1.0],
                         DATA_PROCESSOR=[dict(NAME="transform_points_to_voxels", VOXEL_SIZE=[0.1, 0.1, 0.1])]))


def test_pool_matches_reference_fixture():
    g = np.load(os.path.join(GOLDEN, "second_head_pool.npz"))
    min_x, min_y, vx, vy, ds, grid = g["geometry"]
    out = ops.roi_grid_pool(torch.from_numpy(g["feat"]).cuda(), torch.from_numpy(g["rois"]).cuda(), min_x, min_y, vx, vy, ds, int(grid))
    ref = g["out"]
    np.testing.assert_allclose(out.cpu().numpy(), ref, rtol=0, atol=1e-5 * max(1.0, float(np.abs(ref).max())))


def test_pool_at_toda_shape_matches_torch_and_is_reproducible():
    gen = torch.Generator(device="cuda").manual_seed(0)
    feat = torch.randn((4, 512, 254, 254), device="cuda", generator=gen)
    feat.requires_grad_(True)
    n = 128
    rois = torch.zeros((4, n, 7), device="cuda")
    rois[..., 0:2] = torch.rand((4, n, 2), device="cuda", generator=gen) * 160 - 80       # a few past the +-76.2 m edge
    rois[..., 2] = -1.0
    rois[..., 3:6] = torch.rand((4, n, 3), device="cuda", generator=gen) * torch.tensor([4.0, 1.5, 1.0], device="cuda") + torch.tensor([2.5, 1.2, 1.2], device="cuda")
    rois[..., 6] = torch.rand((4, n), device="cuda", generator=gen) * 2 * np.pi - np.pi
    rois[3, -5:] = 0                                                                         # zero padding of the proposal layer
    args = (-76.2, -76.2, 0.075, 0.075, 8, 7)
    a = ops.roi_grid_pool(feat, rois, *args)
    b = ops.roi_grid_pool(feat, rois, *args)
    assert a.shape == (4 * n, 512, 7, 7) and a.is_contiguous() and not a.requires_grad
    assert torch.equal(a, b)
    with torch.no_grad():
        ref = roi_grid_pool_torch(feat.detach(), rois, *args)
        exact = roi_grid_pool_torch(feat.detach()[:1].double(), rois[:1].double(), *args)        # sample 0 in fp64
    top = float(feat.detach().abs().max())
    err = float((a - ref).abs().max())
    # At W = 254 one ulp of the fp32 sampling position (~1.5e-5 cells) times the map's neighbour differences is ~1e-4: fp32
    # torch and the kernel each sit that far from the fp64 result, in different cells, so they are held to the fp64 yardstick.
    assert err <= 1e-4 * top, err
    err_kernel = float((a[:n].double() - exact).abs().max())
    err_torch = float((ref[:n].double() - exact).abs().max())
    assert err_kernel <= max(1.5 * err_torch, 1e-5 * top), (err_kernel, err_torch)


def _iou_case(rng, b, n, m, n_valid, n_cls=3):
    gt = np.zeros((b, m, 8), np.float32)
    rois = np.zeros((b, n, 7), np.float32)
    for s in range(b):
        k = n_valid[s]
        gt[s, :k, 0:2] = rng.uniform(-15, 15, (k, 2))
        gt[s, :k, 2] = rng.uniform(-1, 0, k)
        gt[s, :k, 3:6] = rng.uniform([3.5, 1.5, 1.4], [4.5, 2.0, 1.8], (k, 3))
        gt[s, :k, 6] = rng.uniform(-np.pi, np.pi, k)
        gt[s, :k, 7] = rng.integers(1, n_cls + 1, k)
        src = gt[s, rng.integers(0, max(k, 1), n), :7] if k else np.zeros((n, 7), np.float32)
        rois[s] = src
        rois[s, :, 0:3] += rng.normal(0, 0.6, (n, 3))
        rois[s, :, 3:6] = np.abs(rois[s, :, 3:6]) * rng.uniform(0.8, 1.2, (n, 3)) + 0.5
        rois[s, :, 6] += rng.uniform(-0.4, 0.4, n)
    labels = rng.integers(1, n_cls + 1, (b, n)).astype(np.int64)
    return rois, labels, gt


def _expected(rois, labels, gt, by_class):
    b, n = labels.shape
    iou, idx = np.zeros((b, n), np.float32), np.zeros((b, n), np.int64)
    for s in range(b):
        k = gt.shape[1] - 1
        while k > 0 and gt[s, k].sum() == 0:
            k -= 1
        g = gt[s, :k + 1] if gt.shape[1] else np.zeros((1, 8), np.float32)
        full = O.boxes_iou3d(rois[s], g[:, :7])
        elig = (g[None, :, 7].astype(np.int64) == labels[s][:, None]) if by_class else np.ones_like(full, bool)
        masked = np.where(elig, full, -1.0)
        best = masked.max(1)
        iou[s] = np.where(best < 0, 0, best)
        idx[s] = np.where(best < 0, 0, masked.argmax(1))
    return iou, idx


@pytest.mark.parametrize("by_class", [True, False])
def test_roi_iou3d_max_matches_oracle(by_class):
    rng = np.random.default_rng(1 if by_class else 2)
    rois, labels, gt = _iou_case(rng, 4, 300, 40, [37, 0, 40, 5])        # trailing zero rows; a sample without gts
    gt[2, 7] = 0                                                          # a zero row inside the valid range
    want_iou, want_idx = _expected(rois, labels, gt, by_class)
    iou, idx = ops.roi_iou3d_max(torch.from_numpy(rois).cuda(), torch.from_numpy(labels).cuda(), torch.from_numpy(gt).cuda(), by_class)
    iou, idx = iou.cpu().numpy(), idx.cpu().numpy()
    np.testing.assert_allclose(iou, want_iou, rtol=0, atol=1e-5)
    pos = want_iou > 1e-4
    assert pos.sum() > 100
    np.testing.assert_array_equal(idx[pos], want_idx[pos])
    assert np.all(iou[1] == 0) and np.all(idx[1] == 0)                     # no valid gt


def test_roi_iou3d_max_ties_no_eligible_gt_and_empty_table():
    box = np.array([1.0, 2.0, -0.5, 4.0, 1.8, 1.6, 0.3], np.float32)
    gt = np.zeros((1, 5, 8), np.float32)
    gt[0, 0, :7], gt[0, 0, 7] = box, 2          # same box twice, different classes ...
    gt[0, 1, :7], gt[0, 1, 7] = box, 1
    gt[0, 2, :7], gt[0, 2, 7] = box, 1          # ... and a tie within class 1
    rois = np.stack([box, box, box + np.array([30, 0, 0, 0, 0, 0, 0], np.float32)])[None]
    labels = np.array([[1, 3, 1]], np.int64)    # class 3: no gt of that class; roi 2 overlaps nothing
    t = lambda a: torch.from_numpy(a).cuda()     # noqa: E731
    iou, idx = ops.roi_iou3d_max(t(rois), t(labels), t(gt), True)
    assert abs(float(iou[0, 0]) - 1.0) < 1e-4 and int(idx[0, 0]) == 1
    assert float(iou[0, 1]) == 0.0 and int(idx[0, 1]) == 0
    assert float(iou[0, 2]) == 0.0 and int(idx[0, 2]) == 1      # eligible gts, all at IoU 0: the first eligible one
    iou, idx = ops.roi_iou3d_max(t(rois), t(labels), t(gt), False)
    assert int(idx[0, 0]) == 0 and int(idx[0, 1]) == 0
    iou, idx = ops.roi_iou3d_max(t(rois), t(labels), torch.zeros((1, 0, 8), device="cuda"), True)
    assert float(iou.abs().sum()) == 0 and int(idx.abs().sum()) == 0


def test_proposal_targets_match_reference_fixture():
    from toda_amd.pcdet.config import AttrDict
    from toda_amd.pcdet.models.roi_heads.target_assigner.proposal_target_layer import ProposalTargetLayer

    g = np.load(os.path.join(GOLDEN, "second_head_targets.npz"))
    ptl = ProposalTargetLayer(AttrDict(TARGET_CONFIG))
    seed = int(g["seed"])
    np.random.seed(seed)
    torch.manual_seed(seed)
    t = lambda k: torch.from_numpy(g[k]).cuda()  # noqa: E731
    out = ptl.forward({"batch_size": 3, "rois": t("rois"), "roi_scores": t("roi_scores"), "roi_labels": t("roi_labels"),
                       "gt_boxes": t("gt_boxes")})
    for k in ("roi_labels", "reg_valid_mask"):
        np.testing.assert_array_equal(out[k].cpu().numpy(), g[f"out_{k}"], err_msg=k)
    for k in ("rois", "roi_scores", "gt_of_rois"):
        np.testing.assert_array_equal(out[k].cpu().numpy(), g[f"out_{k}"], err_msg=k)          # gathers: exact
    for k in ("gt_iou_of_rois", "rcnn_cls_labels"):
        np.testing.assert_allclose(out[k].cpu().numpy(), g[f"out_{k}"], rtol=0, atol=2e-5, err_msg=k)
    assert np.array_equal(out["rcnn_cls_labels"].cpu().numpy() == 0, g["out_rcnn_cls_labels"] == 0)


def _fixture_head():
    from toda_amd.pcdet.models.roi_heads import SECONDHead

    g = np.load(os.path.join(GOLDEN, "second_head_head.npz"))
    head = SECONDHead(input_channels=8, model_cfg=head_cfg(), num_class=1)
    head.load_state_dict({k: torch.from_numpy(g[f"state.{k}"]) for k in head.state_dict()})
    head = head.cuda()
    t = lambda k: torch.from_numpy(g[k]).cuda()  # noqa: E731
    bd = {"batch_size": 3, "rois": t("rois"), "roi_scores": t("roi_scores"), "roi_labels": t("roi_labels"),
          "spatial_features_2d": t("feat"), "dataset_cfg": small_dataset_cfg()}
    return g, head, bd, t


def test_head_forward_loss_and_gradients_match_reference_fixture():
    g, head, bd, t = _fixture_head()
    head.eval()
    with torch.no_grad():
        out = head(dict(bd))
    np.testing.assert_allclose(out["batch_cls_preds"].cpu().numpy(), g["eval_cls"], rtol=1e-4, atol=1e-5)

    head.train()
    seed = int(g["seed"])
    np.random.seed(seed)
    torch.manual_seed(seed)
    head(dict(bd, gt_boxes=t("gt_boxes")))
    np.testing.assert_allclose(head.forward_ret_dict["rcnn_cls_labels"].cpu().numpy(), g["rcnn_cls_labels"], rtol=0, atol=2e-5)
    loss, tb = head.get_loss()
    loss.backward()
    np.testing.assert_allclose(float(loss.detach()), float(g["rcnn_loss_iou"]), rtol=1e-4)
    assert float(tb["rcnn_loss_iou"]) == float(loss)
    for k, p in head.named_parameters():
        ref = g[f"grad.{k}"]
        np.testing.assert_allclose(p.grad.cpu().numpy(), ref, rtol=1e-4, atol=1e-4 * max(1e-3, float(np.abs(ref).max())), err_msg=k)


def _small_kitti_cfg():
    cfg = load_cfg("second_iou_kitti")
    cfg.DATA_CONFIG.SYNTHETIC.NUM_POINTS = 12000
    return cfg


def test_second_iou_kitti_trains_three_steps_and_evaluates():
    from toda_amd.pcdet.datasets import SyntheticLidarDataset
    from toda_amd.pcdet.models import build_network, load_data_to_gpu, prepare_batch_on_gpu

    cfg = _small_kitti_cfg()
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
        for k in ("loss_rpn", "rcnn_loss_iou", "rcnn_loss"):
            assert torch.isfinite(torch.as_tensor(tb[k])), k
        loss.backward()
        grads = [p.grad for p in net.roi_head.parameters() if p.grad is not None]
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
    for p in preds:
        assert set(p) == {"pred_boxes", "pred_scores", "pred_labels", "pred_cls_scores", "pred_iou_scores"}
        n = p["pred_boxes"].shape[0]
        assert all(v.shape[0] == n for v in p.values())
    assert recall["gt"] > 0
    for t in cfg.MODEL.POST_PROCESSING.RECALL_THRESH_LIST:
        assert f"roi_{t}" in recall and f"rcnn_{t}" in recall
        assert 0 <= recall[f"rcnn_{t}"] <= recall["gt"] and 0 <= recall[f"roi_{t}"] <= recall["gt"]


@pytest.mark.parametrize("score_type", ["cls", "weighted_iou_cls", "num_pts_iou_cls"])
def test_post_processing_score_types(score_type):
    from toda_amd.pcdet.config import AttrDict
    from toda_amd.pcdet.datasets import SyntheticLidarDataset
    from toda_amd.pcdet.models import build_network, load_data_to_gpu, prepare_batch_on_gpu

    cfg = _small_kitti_cfg()
    cfg.MODEL.POST_PROCESSING.NMS_CONFIG.SCORE_TYPE = score_type
    cfg.MODEL.POST_PROCESSING.NMS_CONFIG.SCORE_WEIGHTS = AttrDict(dict(iou=0.5, cls=0.5))
    cfg.MODEL.POST_PROCESSING.NMS_CONFIG.SCORE_THRESH = AttrDict(dict(cls=10, iou=100))
    cfg.MODEL.POST_PROCESSING.SCORE_THRESH = 0.0
    ds = SyntheticLidarDataset(cfg.DATA_CONFIG, cfg.CLASS_NAMES, training=False)
    torch.manual_seed(0)
    net = build_network(cfg.MODEL, len(cfg.CLASS_NAMES), ds).cuda().eval()
    batch = ds.collate_batch([ds[0]])
    load_data_to_gpu(batch)
    prepare_batch_on_gpu(batch, net)
    with torch.no_grad():
        preds, _ = net(batch)
    p = preds[0]
    assert p["pred_boxes"].shape[0] > 0
    if score_type == "cls":
        torch.testing.assert_close(p["pred_scores"], p["pred_cls_scores"])
    elif score_type == "weighted_iou_cls":
        torch.testing.assert_close(p["pred_scores"], 0.5 * p["pred_iou_scores"] + 0.5 * p["pred_cls_scores"])


def test_targetmix_config_trains_one_step_through_input_prefetcher():
    from toda_amd.pcdet.datasets import SyntheticMixDataset
    from toda_amd.pcdet.models import InputPrefetcher, build_network

    cfg = load_cfg("toda_stage1_secondiou_targetmix")
    cfg.DATA_CONFIG.SYNTHETIC.NUM_POINTS_SOURCE = 20000
    cfg.DATA_CONFIG.SYNTHETIC.NUM_POINTS_TARGET = 12000
    ds = SyntheticMixDataset(cfg.DATA_CONFIG, cfg.CLASS_NAMES, training=True)
    torch.manual_seed(0)
    np.random.seed(0)
    net = build_network(cfg.MODEL, len(cfg.CLASS_NAMES), ds).cuda().train()
    pre = InputPrefetcher(iter([ds.collate_batch([ds[0], ds[ds.num_source]])]), net, torch.device("cuda", 0))
    try:
        batch = pre.next()
        ret, tb, _ = net(batch)
        loss = ret["loss"]
        loss.backward()
    finally:
        pre.close()
    assert torch.isfinite(loss)
    assert float(sum(p.grad.abs().sum() for p in net.roi_head.parameters() if p.grad is not None)) > 0
    assert batch["spatial_features_2d"].shape[1:] == (512, 254, 254)
