#!/usr/bin/env python
"""Capture golden vectors from the REFERENCE's SECOND-IoU RoI head (build container only, CPU).

    python tests/golden/capture_second_head.py
writes tests/golden/second_head_pool.npz (rotated-RoI grid pool), second_head_targets.npz (ProposalTargetLayer under fixed
seeds) and second_head_head.npz (a small SECONDHead: state dict, eval-mode batch_cls_preds, train-mode loss and gradients).

pcdet/models/roi_heads/{second_head,roi_head_template}.py and roi_heads/target_assigner/proposal_target_layer.py are loaded
by path (capture_reference.setup() / _load).  Their compiled helper iou3d_nms_cuda cannot be built in this image, so
boxes_overlap_bev_gpu and nms_gpu are served by the oracle's C restatements (oracle.boxes_overlap_bev / nms_rotated): the IoU
values in these fixtures are self-referential.  What they pin is the reference's Python logic - the 2 x 3 matrix and
grid_sample call of the pool, the valid-gt count, the class restriction, the order of the random draws of the roi sampler,
the soft IoU labels, the layer order and the loss.  No max-IoU lies within 1e-4 of a sampler threshold (asserted below), so
last-bit differences of a device IoU cannot flip a branch; the rois are given, so no NMS runs.
Only inputs, parameters, seeds and outputs are stored - no reference source.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import capture_reference as CR  # noqa: E402
from capture_reference import EasyDict  # noqa: E402
from oracle import oracle as O  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
THRESH = (0.1, 0.25, 0.55, 0.75)

TARGET_CONFIG = dict(BOX_CODER="ResidualCoder", ROI_PER_IMAGE=32, FG_RATIO=0.5, SAMPLE_ROI_BY_EACH_CLASS=True,
                     CLS_SCORE_TYPE="roi_iou", CLS_FG_THRESH=0.75, CLS_BG_THRESH=0.25, CLS_BG_THRESH_LO=0.1,
                     HARD_BG_RATIO=0.8, REG_FG_THRESH=0.55)
# pool geometry: BEV map of W x H cells of (voxel x DOWNSAMPLE_RATIO) metres starting at (MIN_X, MIN_Y)
MIN_X, MIN_Y, VOXEL, DS, GRID = -4.0, -5.0, 0.1, 4, 7


def head_cfg(in_channel=8, dp_ratio=0.0, iou_loss="BinaryCrossEntropy"):
    return EasyDict(dict(
        NAME="SECONDHead", CLASS_AGNOSTIC=True, SHARED_FC=[16, 16], IOU_FC=[16, 16], DP_RATIO=dp_ratio,
        NMS_CONFIG=dict(TRAIN=dict(NMS_TYPE="nms_gpu", MULTI_CLASSES_NMS=False, NMS_PRE_MAXSIZE=9000, NMS_POST_MAXSIZE=512, NMS_THRESH=0.8),
                        TEST=dict(NMS_TYPE="nms_gpu", MULTI_CLASSES_NMS=False, NMS_PRE_MAXSIZE=1024, NMS_POST_MAXSIZE=100, NMS_THRESH=0.7)),
        ROI_GRID_POOL=dict(GRID_SIZE=GRID, IN_CHANNEL=in_channel, DOWNSAMPLE_RATIO=DS),
        TARGET_CONFIG=TARGET_CONFIG,
        LOSS_CONFIG=dict(IOU_LOSS=iou_loss, LOSS_WEIGHTS=dict(rcnn_iou_weight=1.0, code_weights=[1.0] * 7))))


def dataset_cfg():
    return EasyDict(dict(POINT_CLOUD_RANGE=[MIN_X, MIN_Y, -3.0, 6.0, 5.0, 1.0],
                         DATA_PROCESSOR=[dict(NAME="transform_points_to_voxels", VOXEL_SIZE=[VOXEL, VOXEL, 0.1])]))


def setup():
    CR.setup()
    A = CR.ALIAS
    for name in (f"{A}.models.roi_heads", f"{A}.models.roi_heads.target_assigner"):
        CR._pkg(name)
    iu = sys.modules[f"{A}.ops.iou3d_nms.iou3d_nms_cuda"]

    def boxes_overlap_bev_gpu(a, b, out):
        out.copy_(torch.from_numpy(O.boxes_overlap_bev(a.numpy(), b.numpy())))
        return 1

    def nms_gpu(boxes, keep, thresh):
        k = O.nms_rotated(boxes.numpy(), thresh)
        keep[:len(k)] = torch.from_numpy(k)
        return len(k)

    iu.boxes_overlap_bev_gpu, iu.nms_gpu = boxes_overlap_bev_gpu, nms_gpu
    torch.cuda.FloatTensor = lambda size: torch.zeros(size)      # the reference allocates its IoU outputs this way
    M = {}
    M["ptl"] = CR._load(f"{A}.models.roi_heads.target_assigner.proposal_target_layer",
                        "pcdet/models/roi_heads/target_assigner/proposal_target_layer.py")
    M["template"] = CR._load(f"{A}.models.roi_heads.roi_head_template", "pcdet/models/roi_heads/roi_head_template.py")
    M["second_head"] = CR._load(f"{A}.models.roi_heads.second_head", "pcdet/models/roi_heads/second_head.py")
    return M


def rois_near(rng, gt, n, spread):
    """n rois jittered around the gts (x, y, z by `spread` metres, sizes by +-10 %, heading by +-0.15 rad)."""
    src = gt[rng.integers(0, len(gt), n)]
    out = src.copy()
    out[:, 0:3] += rng.normal(0, spread, (n, 3))
    out[:, 3:6] *= rng.uniform(0.9, 1.1, (n, 3))
    out[:, 6] += rng.uniform(-0.15, 0.15, n)
    return out.astype(np.float32)


def cap_pool(M):
    rng = np.random.default_rng(11)
    feat = rng.standard_normal((2, 16, 20, 24)).astype(np.float32)
    n = 9
    rois = np.zeros((2, n, 7), np.float32)
    rois[:, :, 0] = rng.uniform(-3.0, 5.0, (2, n))
    rois[:, :, 1] = rng.uniform(-4.5, 2.5, (2, n))
    rois[:, :, 2] = rng.uniform(-1, 0, (2, n))
    rois[:, :, 3:6] = rng.uniform(0.6, 4.5, (2, n, 3))
    rois[:, :, 6] = np.linspace(-np.pi, np.pi, 2 * n).reshape(2, n)
    rois[0, 0, 0:2] = [5.3, 2.7]              # partly outside the map (far corner)
    rois[1, 1, 0:2] = [-4.2, -5.1]            # partly outside (origin corner)
    rois[1, 2, 0:2] = [9.0, 9.0]              # entirely outside
    rois[1, -1] = 0                           # zero-padded roi
    head = M["second_head"].SECONDHead(input_channels=16, model_cfg=head_cfg(in_channel=16), num_class=1)
    out = head.roi_grid_pool({"batch_size": 2, "rois": torch.from_numpy(rois), "spatial_features_2d": torch.from_numpy(feat),
                              "dataset_cfg": dataset_cfg()})
    np.savez_compressed(os.path.join(OUT, "second_head_pool.npz"), feat=feat, rois=rois, out=out.numpy(),
                        geometry=np.array([MIN_X, MIN_Y, VOXEL, VOXEL, DS, GRID], np.float64))
    print("pool", out.shape, float(np.abs(out.numpy()).max()))


def target_inputs(seed):
    """3 samples: mixed fg / bg with a class (3) that has rois but no gt; all-zero gts (bg only); rois that nearly all sit on
    their gts (fg-heavy: more fg than FG_RATIO admits).  The reference's fg-only branch raises (torch.cat of a tensor and a
    Python list), so it has no fixture; tests/test_second_iou_host.py pins its random draw instead."""
    rng = np.random.default_rng(seed)
    n, m = 40, 6
    gt = np.zeros((3, m, 8), np.float32)
    base = np.stack([rng.uniform(-20, 20, 5), rng.uniform(-20, 20, 5), rng.uniform(-1, 0, 5), rng.uniform(3.5, 4.5, 5),
                     rng.uniform(1.6, 2.0, 5), rng.uniform(1.4, 1.7, 5), rng.uniform(-np.pi, np.pi, 5)], 1).astype(np.float32)
    gt[0, :4, :7], gt[0, :4, 7] = base[:4], [1, 2, 1, 2]
    gt[2, :5, :7], gt[2, :5, 7] = base, [1, 1, 2, 2, 1]
    rois = np.zeros((3, n, 7), np.float32)
    labels = np.zeros((3, n), np.int64)
    near = rois_near(rng, gt[0, :4, :7], 24, 0.1)
    far = near[:16].copy()
    far[:, 0:2] += rng.uniform(0.5, 4, (16, 2)) * rng.choice([-1, 1], (16, 2))
    rois[0] = np.concatenate([near, far], 0)
    labels[0] = np.where(rng.uniform(0, 1, n) < 0.8, np.tile(gt[0, :4, 7], 10).astype(np.int64), 3)     # class 3: rois, no gt
    rois[1] = rois_near(rng, base, n, 2.0)
    labels[1] = rng.integers(1, 3, n)
    src = rng.integers(0, 5, n)
    rois[2] = gt[2, src, :7]
    rois[2, :, 0:2] += rng.normal(0, 0.03, (n, 2))
    rois[2, -4:, 0:2] += 10.0                              # four background rois
    labels[2] = gt[2, src, 7].astype(np.int64)
    scores = rng.uniform(0, 1, (3, n)).astype(np.float32)
    return rois, scores, labels, gt


def run_targets(M, rois, scores, labels, gt, seed):
    ptl = M["ptl"].ProposalTargetLayer(EasyDict(TARGET_CONFIG))
    record = {"max_iou": [], "picks": []}
    get_max, subsample = ptl.get_max_iou_with_same_class, ptl.subsample_rois

    def get_max_rec(**kw):
        mo, ga = get_max(**kw)
        record["max_iou"].append(mo.numpy().copy())
        return mo, ga

    def subsample_rec(max_overlaps):
        idx = subsample(max_overlaps=max_overlaps)
        record["picks"].append(idx.numpy().copy())
        return idx

    ptl.get_max_iou_with_same_class, ptl.subsample_rois = get_max_rec, subsample_rec
    np.random.seed(seed)
    torch.manual_seed(seed)
    out = ptl.forward({"batch_size": 3, "rois": torch.from_numpy(rois), "roi_scores": torch.from_numpy(scores),
                       "roi_labels": torch.from_numpy(labels), "gt_boxes": torch.from_numpy(gt)})
    return out, record


def margin_ok(table):
    return all(np.abs(table - t).min() > 1e-4 for t in THRESH)


def cap_targets(M):
    seed = 0
    while True:
        rois, scores, labels, gt = target_inputs(100 + seed)
        out, rec = run_targets(M, rois, scores, labels, gt, 7)
        if margin_ok(np.stack(rec["max_iou"])):
            break
        seed += 1
        assert seed < 50, "no input seed keeps the max-IoUs off the thresholds"
    tables = np.stack(rec["max_iou"])
    fg = (tables >= 0.55).sum(1)
    print("targets: input seed", 100 + seed, "fg per sample", fg.tolist(), "bg per sample", (tables < 0.55).sum(1).tolist())
    np.savez_compressed(os.path.join(OUT, "second_head_targets.npz"), rois=rois, roi_scores=scores, roi_labels=labels, gt_boxes=gt,
                        seed=np.int64(7), max_iou=tables, picks=np.stack(rec["picks"]),
                        **{f"out_{k}": v.numpy() for k, v in out.items()})


def cap_head(M):
    rng = np.random.default_rng(5)
    torch.manual_seed(3)
    cfg = head_cfg(in_channel=8, dp_ratio=0.0)
    head = M["second_head"].SECONDHead(input_channels=8, model_cfg=cfg, num_class=1)
    for m in head.modules():                      # non-trivial BN affine parameters and running statistics
        if isinstance(m, torch.nn.BatchNorm1d):
            m.weight.data.uniform_(0.5, 1.5)
            m.bias.data.uniform_(-0.2, 0.2)
            m.running_mean.uniform_(-0.1, 0.1)
            m.running_var.uniform_(0.5, 1.5)
    state = {k: v.detach().numpy().copy() for k, v in head.state_dict().items()}
    rois, scores, labels, gt = target_inputs(100)
    rois[:, :, 0:2] = rois[:, :, 0:2] / 8.0          # into the small map's extent (the targets fixture's geometry / 8)
    gt[:, :, 0:2] = gt[:, :, 0:2] / 8.0
    for b in range(3):
        rois[b] = np.where(np.all(rois[b] == 0, axis=1, keepdims=True), 0, rois[b])
    feat = rng.standard_normal((3, 8, 20, 24)).astype(np.float32)
    # eval
    head.eval()
    bd = {"batch_size": 3, "rois": torch.from_numpy(rois), "roi_scores": torch.from_numpy(scores), "roi_labels": torch.from_numpy(labels),
          "spatial_features_2d": torch.from_numpy(feat), "dataset_cfg": dataset_cfg()}
    with torch.no_grad():
        eval_cls = head(dict(bd))["batch_cls_preds"].numpy()
    # train (DP_RATIO 0): sampler under fixed seeds, loss, parameter gradients
    head.train()
    np.random.seed(9)
    torch.manual_seed(9)
    head(dict(bd, gt_boxes=torch.from_numpy(gt)))
    loss, _ = head.get_box_iou_layer_loss(head.forward_ret_dict)
    loss.backward()
    grads = {f"grad.{k}": p.grad.numpy().copy() for k, p in head.named_parameters()}
    tables = []
    with torch.no_grad():
        out, rec = run_targets(M, rois, scores, labels, gt, 9)
        tables = np.stack(rec["max_iou"])
    assert margin_ok(tables), "head fixture: a max-IoU sits on a sampler threshold"
    keys = np.array(list(state.keys()))
    np.savez_compressed(os.path.join(OUT, "second_head_head.npz"), rois=rois, roi_scores=scores, roi_labels=labels, gt_boxes=gt, feat=feat,
                        seed=np.int64(9), keys=keys, eval_cls=eval_cls, rcnn_loss_iou=np.float32(loss.item()),
                        rcnn_cls_labels=head.forward_ret_dict["rcnn_cls_labels"].numpy(),
                        **{f"state.{k}": v for k, v in state.items()}, **grads)
    print("head: keys", len(keys), "loss", loss.item())


def main():
    M = setup()
    cap_pool(M)
    cap_targets(M)
    cap_head(M)


if __name__ == "__main__":
    main()
