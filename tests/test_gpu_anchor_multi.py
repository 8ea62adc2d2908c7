"""toda_anchor_assign on the GPU: against the torch route of AxisAlignedTargetAssigner (the reference's loop) on screened
inputs (tests/anchor_multi_cases.py), against the reference-captured c1_pointpillar_chain targets in single-head order, at its
edge shapes and at the full nuScenes shape; AnchorHeadMulti trains on both new configs and evaluates through the per-class NMS.

Positive target rows: the kernel's maximum error against a float64 evaluation of the encode formula may be at most twice the
torch fp32 route's own maximum error against the same values (device logf and torch's log are each good to an ulp or two
on O(1) targets); both errors are printed."""
import os

import numpy as np
import pytest
import torch

from tests import anchor_multi_cases as cases

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RANGE16 = [0.0, -8.0, -3.0, 16.0, 8.0, 1.0]


def both_routes(assigner, anchors, gt):
    dev_anchors = [a.cuda() for a in anchors]
    g = torch.from_numpy(gt).cuda()
    hip = assigner.assign_targets_hip(dev_anchors, g)
    ref = assigner.assign_targets_torch(dev_anchors, g.clone())
    return hip, ref


def positive_rows_f64(anchors, gt, specs, labels, multihead, sincos):
    """(row mask [B, A], float64 targets of those rows in row order) from the best gt of every positive anchor."""
    out = []
    offs = np.cumsum([0] + [int(np.prod(a.shape[:-1])) for a in anchors])
    flat = cases.flat_anchors(anchors, multihead).numpy()
    per_loc = [int(a.shape[3] * a.shape[4]) for a in anchors]
    for b in range(gt.shape[0]):
        rows = np.nonzero(labels[b] > 0)[0]
        if multihead:
            cls_of = np.searchsorted(offs, rows, side="right") - 1
        else:
            cls_of = np.searchsorted(np.cumsum([0] + per_loc), rows % sum(per_loc), side="right") - 1
        for r, c in zip(rows, cls_of):
            sel = gt[b, :, -1].astype(np.int64) == c + 1
            iou = cases.iou_matrix(flat[r:r + 1], gt[b, sel], np.float32)
            out.append(cases.encode_f64(gt[b, sel][int(iou.argmax(1)[0])][None, :-1], flat[r:r + 1], sincos)[0])
    return labels > 0, np.asarray(out, np.float64)


def compare(assigner, anchors, gt, specs, multihead, sincos, expect_positives=True):
    hip, ref = both_routes(assigner, anchors, gt)
    lh, lr = hip["box_cls_labels"].cpu().numpy(), ref["box_cls_labels"].cpu().numpy()
    assert lh.dtype == np.int32 and np.array_equal(lh, lr), f"{int((lh != lr).sum())} labels differ"
    assert np.array_equal(hip["reg_weights"].cpu().numpy(), ref["reg_weights"].cpu().numpy())
    th, tr = hip["box_reg_targets"].cpu().numpy(), ref["box_reg_targets"].cpu().numpy()
    assert th.shape == tr.shape
    pos = lh > 0
    assert not th[~pos].view(np.uint32).any(), "a non-positive target row is not bit-zero"
    if expect_positives:
        assert pos.any()
    if pos.any():
        _, want = positive_rows_f64(anchors, gt, specs, lh, multihead, sincos)
        err_hip, err_torch = np.abs(th[pos] - want).max(), np.abs(tr[pos] - want).max()
        print(f"positives {int(pos.sum())}: max |kernel - f64| {err_hip:.3e}, max |torch fp32 - f64| {err_torch:.3e}")
        assert err_hip <= 2 * err_torch, (err_hip, err_torch)
    return hip


@pytest.mark.parametrize("multihead", [False, True])
@pytest.mark.parametrize("code_size,sincos,n_extra", [(7, False, 0), (9, True, 2)])
def test_kernel_matches_torch_route_small_maps(multihead, code_size, sincos, n_extra):
    assigner, anchors = cases.make_assigner(cases.SMALL4, (16, 16), RANGE16, multihead, code_size, sincos)
    # an empty sample, one gt, and a full sample; class 2 (Cyclist) has no gt anywhere; trailing padding
    def make(seed):
        gt = cases.draw_gt(seed, cases.SMALL4, RANGE16, 3, 12, n_extra=n_extra, counts=[0, 1, 9], class_pool=[0, 1, 3])
        gt[2, 8, :2] = [40.0, 40.0]                  # a gt outside every anchor: touches nothing, forces nothing
        return gt

    gt = cases.first_screened(make, 11, anchors, cases.SMALL4)
    hip = compare(assigner, anchors, gt, cases.SMALL4, multihead, sincos)
    assert hip["box_reg_targets"].shape[-1] == code_size + (1 if sincos else 0)
    assert int((hip["box_cls_labels"][0] != 0).sum()) == 0          # the empty sample: all background


def test_kernel_matches_the_reference_fixture_in_both_orders():
    """toda_anchor_assign on the inputs of anchor_multi_assign.npz against the reference's own outputs: labels and weights
    equal, zero rows bit-zero, positive rows at the C1 chain's target tolerance; code size 7 and 9 + sin/cos."""
    cases.check_assign_fixture("hip", "cuda")
    cases.check_assign_fixture("torch", "cuda")


def test_head_matches_the_reference_fixture():
    """AnchorHeadMulti forward, decode and the class / box / direction losses against anchor_multi_head.npz, targets through
    the kernel (auto routes a multi-head to it); tol 2.0 as the C1 chain and BEV fixtures on the GPU."""
    cases.check_head_fixture("cuda", tol=2.0)


def test_multi_class_post_processing_matches_the_reference_fixture():
    cases.check_nms_fixture("cuda")


def test_no_gt_rows_at_all_and_strided_tables_are_refused():
    from toda_amd import ops

    assigner, anchors = cases.make_assigner(cases.KITTI3, (16, 16), RANGE16, True)
    dev = [a.cuda() for a in anchors]
    out = assigner.assign_targets_hip(dev, torch.zeros((2, 0, 8), device="cuda"))          # M = 0: all background
    assert int(out["box_cls_labels"].abs().sum()) == 0 and not out["box_reg_targets"].view(torch.int32).any()
    slot = torch.tensor([-1, 0, 1, 2], dtype=torch.int32, device="cuda")
    gt = torch.zeros((1, 2, 8), device="cuda")
    view = [torch.cat([a, a], dim=-1)[..., :7] for a in dev]                               # right shape, wrong strides
    with pytest.raises(RuntimeError, match="contiguous"):
        ops.anchor_assign(view, gt, slot, [0.6, 0.5, 0.5], [0.45, 0.35, 0.35], 7, multihead=True)
    with pytest.raises(RuntimeError, match="slot_of"):
        ops.anchor_assign(dev, gt, slot.long(), [0.6, 0.5, 0.5], [0.45, 0.35, 0.35], 7, multihead=True)


def test_single_head_order_matches_reference_capture(monkeypatch):
    """TODA_ANCHOR_ASSIGN=hip on AnchorHeadSingle: the reference's own labels / targets / weights of c1_pointpillar_chain,
    at the tolerance the chain test uses for them, and the torch route's labels."""
    from tests.test_golden_reference import C1_HEAD, load
    from toda_amd.pcdet.config import AttrDict
    from toda_amd.pcdet.models.dense_heads import AnchorHeadSingle

    g = load("c1_pointpillar_chain")
    head = AnchorHeadSingle(AttrDict(C1_HEAD), 48, 3, ["Car", "Pedestrian", "Cyclist"], np.array([48, 48, 1]), g["pc_range"],
                            predict_boxes_when_training=False).cuda()
    gt = torch.from_numpy(g["gt"].copy()).cuda()
    monkeypatch.setenv("TODA_ANCHOR_ASSIGN", "torch")
    assert head.target_assigner.route(gt) == "torch"
    ref = head.assign_targets(gt.clone())
    monkeypatch.delenv("TODA_ANCHOR_ASSIGN")
    assert head.target_assigner.route(gt) == "torch"             # auto: AnchorHeadSingle stays where it was
    monkeypatch.setenv("TODA_ANCHOR_ASSIGN", "hip")
    assert head.target_assigner.route(gt) == "hip"
    out = head.assign_targets(gt)
    assert np.array_equal(out["box_cls_labels"].cpu().numpy(), ref["box_cls_labels"].cpu().numpy())
    assert np.array_equal(out["box_cls_labels"].cpu().numpy(), g["box_cls_labels"])
    np.testing.assert_allclose(out["box_reg_targets"].cpu().numpy(), g["box_reg_targets"], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(out["reg_weights"].cpu().numpy(), g["reg_weights"], rtol=0, atol=0)


def test_edge_anchor_count_not_a_multiple_of_the_tile():
    assigner, anchors = cases.make_assigner(cases.KITTI3, (15, 13), [0.0, -6.5, -3.0, 15.0, 6.5, 1.0], True)
    assert (15 * 13 * 2) % 256 != 0
    gt = cases.screened_gt(21, anchors, cases.KITTI3, [0.0, -6.5, -3.0, 15.0, 6.5, 1.0], 2, 6)
    compare(assigner, anchors, gt, cases.KITTI3, True, False)


@pytest.mark.parametrize("multihead", [False, True])
def test_edge_more_gts_of_one_class_than_a_wave_and_than_one_chunk(multihead):
    """600 gt rows = three 256-row LDS chunks.  Sample 0: 70 gts of one class (more than the 64 lanes of a wave), half of
    them in the second chunk behind a stretch of zero rows; sample 1: 20 mixed gts across the first chunk boundary."""
    rng = [0.0, -24.0, -3.0, 48.0, 24.0, 1.0]
    assigner, anchors = cases.make_assigner(cases.KITTI3, (48, 48), rng, multihead)

    def make(seed):
        gt = np.zeros((2, 600, 8), np.float32)
        many = cases.draw_gt(seed, cases.KITTI3, rng, 1, 70, class_pool=[1])[0]
        gt[0, 0:35], gt[0, 300:335] = many[:35], many[35:]
        gt[1, 246:266] = cases.draw_gt(seed + 1, cases.KITTI3, rng, 1, 20)[0]
        return gt

    gt = cases.first_screened(make, 31, anchors, cases.KITTI3)
    assert int((gt[0, :, -1] == 2).sum()) == 70
    compare(assigner, anchors, gt, cases.KITTI3, multihead, False)


def test_edge_no_gt_in_the_batch_one_class_and_one_row():
    assigner, anchors = cases.make_assigner(cases.KITTI3, (16, 16), RANGE16, True)
    hip = compare(assigner, anchors, np.zeros((2, 5, 8), np.float32), cases.KITTI3, True, False, expect_positives=False)
    assert int(hip["box_cls_labels"].abs().sum()) == 0 and int(hip["reg_weights"].abs().sum()) == 0
    one, one_anchors = cases.make_assigner(cases.KITTI3[:1], (16, 16), RANGE16, True)
    gt = cases.screened_gt(41, one_anchors, cases.KITTI3[:1], RANGE16, 2, 1)          # one class only, M = 1
    compare(one, one_anchors, gt, cases.KITTI3[:1], True, False)


def test_edge_identical_gts_take_the_lowest_index():
    assigner, anchors = cases.make_assigner(cases.KITTI3, (16, 16), RANGE16, True, code_size=9, sincos=True)
    def make(seed):
        gt = cases.draw_gt(seed, cases.KITTI3, RANGE16, 1, 4, n_extra=2, class_pool=[0])
        gt[0, 2, :7] = gt[0, 0, :7]                  # same box, different velocity: the targets tell which gt won
        gt[0, 3, :7] = gt[0, 0, :7]
        return gt

    gt = cases.first_screened(make, 51, anchors, cases.KITTI3)
    hip = compare(assigner, anchors, gt, cases.KITTI3, True, True)
    flat = cases.flat_anchors(anchors, True).numpy()
    iou = cases.iou_matrix(flat[:512], gt[0, :, :], np.float32)
    rows = np.nonzero((iou[:, 0] > 0) & (iou[:, 0] >= iou[:, 1]) & (hip["box_cls_labels"][0, :512].cpu().numpy() > 0))[0]
    assert len(rows) > 0
    np.testing.assert_array_equal(hip["box_reg_targets"][0, rows, 8:10].cpu().numpy(), np.tile(gt[0, 0, 7:9], (len(rows), 1)))


def test_edge_square_anchor_forces_both_rotations():
    specs = [cases.SMALL4[3]]
    assigner, anchors = cases.make_assigner(specs, (16, 16), RANGE16, True)
    gt = np.zeros((1, 2, 8), np.float32)
    gt[0, 0] = [5.3, 1.2, -0.5, 0.5, 0.5, 1.0, 0.2, 1]                # small: below matched everywhere, positives only by force
    assert not cases.screening_failures(anchors, gt, specs)
    hip = compare(assigner, anchors, gt, specs, True, False)
    lab = hip["box_cls_labels"][0].cpu().numpy().reshape(2, 16 * 16)    # (rotation, location)
    assert lab[0].max() == 1 and np.array_equal(lab[0] > 0, lab[1] > 0)


def test_full_nuscenes_shape_labels_reproducible_and_sync_free():
    """B 4, 128 x 128, 10 classes x 2 rotations = 327 680 anchors per sample, 40 gts per sample."""
    rng = [-51.2, -51.2, -5.0, 51.2, 51.2, 3.0]
    assigner, anchors = cases.make_assigner(cases.NUSC10, (128, 128), rng, True, code_size=9, sincos=True)
    assert sum(int(np.prod(a.shape[:-1])) for a in anchors) == 327680
    gt = cases.screened_gt(61, anchors, cases.NUSC10, rng, 4, 40, n_extra=2)
    dev_anchors, g = [a.cuda() for a in anchors], torch.from_numpy(gt).cuda()
    ref = assigner.assign_targets_torch(dev_anchors, g.clone())
    first = assigner.assign_targets_hip(dev_anchors, g)               # also places the class table on the device
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        second = assigner.assign_targets_hip(dev_anchors, g)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.equal(first["box_cls_labels"], ref["box_cls_labels"])
    assert torch.equal(first["reg_weights"], ref["reg_weights"])
    assert int((first["box_cls_labels"] > 0).sum()) >= 4 * 40
    for k in first:
        assert torch.equal(first[k].view(torch.int32), second[k].view(torch.int32)), k
    pos = first["box_cls_labels"] > 0
    torch.testing.assert_close(first["box_reg_targets"][pos], ref["box_reg_targets"][pos], rtol=1e-5, atol=1e-6)
    assert not first["box_reg_targets"][~pos].view(torch.int32).any()


def load_cfg(name):
    from toda_amd.pcdet.config import AttrDict, cfg_from_yaml_file

    cfg = AttrDict()
    cfg_from_yaml_file(os.path.join(ROOT, "toda_amd", "tools", "cfgs", "models", f"{name}.yaml"), cfg)
    return cfg


@pytest.mark.parametrize("name,points", [("cbgs_pp_multihead_nuscenes", 20000), ("second_multihead_kitti", 12000)])
def test_new_configs_train_five_steps_and_evaluate(name, points):
    from toda_amd.pcdet.datasets import SyntheticLidarDataset
    from toda_amd.pcdet.models import build_network, load_data_to_gpu, prepare_batch_on_gpu
    from toda_amd.pcdet.models.dense_heads import AnchorHeadMulti

    cfg = load_cfg(name)
    cfg.DATA_CONFIG.SYNTHETIC.NUM_POINTS = points
    ds = SyntheticLidarDataset(cfg.DATA_CONFIG, cfg.CLASS_NAMES, training=True)
    torch.manual_seed(0)
    np.random.seed(0)
    net = build_network(cfg.MODEL, len(cfg.CLASS_NAMES), ds).cuda().train()
    assert isinstance(net.dense_head, AnchorHeadMulti) and net.dense_head.target_assigner.use_multihead
    opt = torch.optim.Adam(net.parameters(), lr=1e-3)
    losses = []
    for step in range(5):
        batch = ds.collate_batch([ds[0], ds[1]])                       # one repeated batch
        prepare_batch_on_gpu(batch, net)
        assert net.dense_head.target_assigner.route(batch["gt_boxes"]) == "hip"
        opt.zero_grad()
        ret, tb, _ = net(batch)
        loss = ret["loss"]
        assert torch.isfinite(loss), (step, tb)
        loss.backward()
        if step == 0:
            missing = [k for k, p in net.named_parameters() if p.requires_grad and p.grad is None]
            assert not missing, missing
        opt.step()
        losses.append(float(loss.detach()))
    print(name, "losses", losses)
    assert losses[-1] < losses[0], losses

    net.eval()
    test_ds = SyntheticLidarDataset(cfg.DATA_CONFIG, cfg.CLASS_NAMES, training=False)
    batch = test_ds.collate_batch([test_ds[0], test_ds[1]])
    load_data_to_gpu(batch)
    prepare_batch_on_gpu(batch, net)
    with torch.no_grad():
        preds, recall = net(batch)
    assert len(preds) == 2 and recall["gt"] > 0
    for p in preds:
        n = p["pred_boxes"].shape[0]
        assert p["pred_scores"].shape[0] == n and p["pred_labels"].shape[0] == n
        if n:
            assert int(p["pred_labels"].min()) >= 1 and int(p["pred_labels"].max()) <= len(cfg.CLASS_NAMES)
            assert float(p["pred_scores"].min()) >= cfg.MODEL.POST_PROCESSING.SCORE_THRESH


def test_multi_class_post_processing_keeps_per_class_maxima():
    """Two heads' scores over well separated and duplicated boxes: per class the duplicates collapse to the best one, the
    labels come from the heads' mapping, and no class exceeds NMS_POST_MAXSIZE."""
    from toda_amd.pcdet.config import AttrDict
    from toda_amd.pcdet.models.detectors.detector3d_template import Detector3DTemplate

    class Stub(Detector3DTemplate):
        def __init__(self):
            torch.nn.Module.__init__(self)
            self.num_class = 3
            self.model_cfg = AttrDict(dict(POST_PROCESSING=dict(
                RECALL_THRESH_LIST=[0.5], SCORE_THRESH=0.3, OUTPUT_RAW_SCORE=False,
                NMS_CONFIG=dict(MULTI_CLASSES_NMS=True, NMS_TYPE="nms_gpu", NMS_THRESH=0.1, NMS_PRE_MAXSIZE=100, NMS_POST_MAXSIZE=2))))

    n = 6
    boxes = torch.zeros(1, 2 * n, 7)
    for i in range(n):                                   # per head: pairs of identical boxes 10 m apart
        boxes[0, i] = torch.tensor([10.0 * (i // 2), 0.0, 0.0, 4.0, 2.0, 1.5, 0.1])
        boxes[0, n + i] = torch.tensor([10.0 * (i // 2), 30.0, 0.0, 1.0, 1.0, 1.5, 0.0])
    head0 = torch.tensor([[0.9], [0.8], [0.7], [0.2], [0.6], [0.5]]).unsqueeze(0)                       # class 2
    head1 = torch.tensor([[0.9, 0.1], [0.1, 0.8], [0.7, 0.1], [0.1, 0.1], [0.6, 0.95], [0.5, 0.4]]).unsqueeze(0)  # classes 1, 3
    batch = {"batch_size": 1, "batch_box_preds": boxes.cuda(), "batch_cls_preds": [head0.cuda(), head1.cuda()],
             "cls_preds_normalized": True, "multihead_label_mapping": [torch.tensor([2]).cuda(), torch.tensor([1, 3]).cuda()]}
    preds, _ = Stub().post_processing(batch)
    p = {k: v.cpu() for k, v in preds[0].items()}
    assert p["pred_labels"].tolist() == [2, 2, 1, 1, 3, 3]
    torch.testing.assert_close(p["pred_scores"], torch.tensor([0.9, 0.7, 0.9, 0.7, 0.95, 0.8]))
    assert p["pred_boxes"][:, 1].tolist() == [0.0, 0.0, 30.0, 30.0, 30.0, 30.0]
    assert p["pred_boxes"][:, 0].tolist() == [0.0, 10.0, 0.0, 10.0, 20.0, 0.0]
