#!/usr/bin/env python
"""Capture the multi-head anchor fixtures from the REFERENCE's own Python (build container only).

    python tests/golden/capture_anchor_multi.py

writes tests/golden/anchor_multi_assign.npz (AxisAlignedTargetAssigner in both anchor orders, code size 7 and 9 + sin/cos),
anchor_multi_head.npz (a two-head AnchorHeadMulti with separate regression branches: forward, decode, the three losses) and
anchor_multi_nms.npz (Detector3DTemplate.post_processing with MULTI_CLASSES_NMS over two heads' score lists).

The reference files (anchor_head_multi.py, anchor_head_template.py, the target assigner, model_nms_utils.py,
box_coder_utils.py, detector3d_template.py) are loaded by path with the stub / _load recipe of capture_reference.py.  The
reference's compiled `iou3d_nms_cuda.nms_gpu` cannot be built in this image; the oracle's rotated NMS (oracle_nms_rotated,
greedy over boxes sorted by score, the same rule) stands in for it, so what anchor_multi_nms.npz pins is the reference's
Python: masks, top-k, NMS_POST_MAXSIZE, label mapping and the order of the output rows.  Only inputs, weights, parameters and
outputs are stored - no reference source.

Screening of the assigner's gt sets is a condition, not a mask: a seed is rejected and the next one drawn unless no anchor's
best IoU lies within 1e-4 of a threshold and each gt's set of maximal anchors is the same in float64 and float32
(tests/anchor_multi_cases.py); tests/test_anchor_multi_host.py recomputes both from the committed inputs.
"""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import capture_reference as CR  # noqa: E402
from oracle import oracle as O  # noqa: E402
from tests import anchor_multi_cases as cases  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
ED = CR.EasyDict
RANGE16 = [0.0, -8.0, -3.0, 16.0, 8.0, 1.0]


def setup():
    L = CR.setup()
    A = CR.ALIAS
    iu = sys.modules[f"{A}.ops.iou3d_nms.iou3d_nms_cuda"]

    def nms_gpu(boxes, keep, thresh):              # boxes arrive sorted by score; fills keep, returns the count
        kept = O.nms_rotated(boxes.numpy(), thresh)
        keep[:len(kept)] = torch.from_numpy(kept)
        return len(kept)

    iu.nms_gpu = nms_gpu
    sys.modules[f"{A}.models.backbones_2d"].BaseBEVBackbone = L["base_bev_backbone"].BaseBEVBackbone
    L["anchor_head_multi"] = CR._load(f"{A}.models.dense_heads.anchor_head_multi", "pcdet/models/dense_heads/anchor_head_multi.py")
    sp = types.ModuleType(f"{A}.utils.spconv_utils")
    sp.find_all_spconv_keys = lambda *a, **k: set()
    sys.modules[sp.__name__] = sp
    setattr(sys.modules[f"{A}.utils"], "spconv_utils", sp)
    for name in (f"{A}.models.roi_heads", f"{A}.models.backbones_3d.pfe", f"{A}.models.detectors"):
        CR._pkg(name)
    L["detector3d_template"] = CR._load(f"{A}.models.detectors.detector3d_template", "pcdet/models/detectors/detector3d_template.py")
    L["model_nms_utils"] = sys.modules[f"{A}.models.model_utils.model_nms_utils"]
    L["target_assigner"] = sys.modules[f"{A}.models.dense_heads.target_assigner.axis_aligned_target_assigner"]
    return L


def ref_head_cfg(specs, multihead, code_size, sincos):
    return ED(cases.head_cfg(specs, multihead, code_size, sincos))


def cap_assign(L):
    """16 x 16 map, four classes (the last with a square anchor), batch 3: an empty sample, a sample with one gt, a full one
    with a gt outside every anchor and trailing padding; Cyclist has no gt anywhere."""
    out = {"pc_range": np.asarray(RANGE16, np.float32), "class_names": np.array([s[0] for s in cases.SMALL4])}
    names = [s[0] for s in cases.SMALL4]
    for code_size, sincos, n_extra in ((7, False, 0), (9, True, 2)):
        coder = L["box_coder_utils"].ResidualCoder(code_size=code_size, encode_angle_by_sincos=sincos)
        cfg = ref_head_cfg(cases.SMALL4, False, code_size, sincos)
        anchors, _ = L["anchor_head_template"].AnchorHeadTemplate.generate_anchors(
            cfg.ANCHOR_GENERATOR_CONFIG, grid_size=np.array([16, 16, 1]), point_cloud_range=np.asarray(RANGE16, np.float32),
            anchor_ndim=coder.code_size)

        def make(seed):
            gt = cases.draw_gt(seed, cases.SMALL4, RANGE16, 3, 12, n_extra=n_extra, counts=[0, 1, 9], class_pool=[0, 1, 3])
            gt[2, 8, :2] = [40.0, 40.0]
            return gt

        gt = cases.first_screened(make, 11, anchors, cases.SMALL4)
        tag = f"c{code_size}"
        out[f"{tag}_gt"] = gt
        for k, a in enumerate(anchors):
            out[f"{tag}_anchors{k}"] = a.numpy()
        for multihead in (False, True):
            cfg = ref_head_cfg(cases.SMALL4, multihead, code_size, sincos)
            assigner = L["target_assigner"].AxisAlignedTargetAssigner(cfg, names, coder, match_height=False)
            t = assigner.assign_targets(anchors, torch.from_numpy(gt.copy()))
            order = "multi" if multihead else "single"
            out[f"{tag}_{order}_labels"] = t["box_cls_labels"].numpy()
            out[f"{tag}_{order}_targets"] = t["box_reg_targets"].numpy()
            out[f"{tag}_{order}_weights"] = t["reg_weights"].numpy()
            print("assign", tag, order, "positives", int((t["box_cls_labels"] > 0).sum()), "ignored", int((t["box_cls_labels"] < 0).sum()))
    np.savez_compressed(os.path.join(OUT, "anchor_multi_assign.npz"), **out)


def cap_head(L):
    """Two heads (Car | Pedestrian + Cyclist) behind a shared convolution, separate regression branches with one middle
    convolution, direction classifier, train mode, batch 2 on a 16 x 16 map of 24 channels."""
    names = [s[0] for s in cases.HEAD_SPECS]
    torch.manual_seed(21)
    head = L["anchor_head_multi"].AnchorHeadMulti(ED(cases.head_model_cfg()), 24, 3, names, np.array([16, 16, 1]),
                                                  np.asarray(RANGE16, np.float32), predict_boxes_when_training=True).train()
    for m in head.modules():                       # BatchNorms away from their identity start
        if isinstance(m, torch.nn.BatchNorm2d):
            torch.nn.init.uniform_(m.weight, 0.6, 1.4)
            torch.nn.init.uniform_(m.bias, -0.2, 0.2)
    for h in head.rpn_heads:                       # the direction and last box convolutions away from near-zero outputs
        torch.nn.init.normal_(h.conv_dir_cls.weight, std=0.3)
    w = CR.sd_np(head, "w.")
    keys = np.array(list(head.state_dict().keys()))
    g = torch.Generator().manual_seed(22)
    x = torch.randn((2, 24, 16, 16), generator=g)
    gt = cases.first_screened(lambda s: cases.draw_gt(s, cases.HEAD_SPECS, RANGE16, 2, 7, counts=[7, 4]), 23, head.anchors, cases.HEAD_SPECS)
    d = head({"spatial_features_2d": x, "gt_boxes": torch.from_numpy(gt.copy()), "batch_size": 2})
    loss, tb = head.get_loss()
    fr = head.forward_ret_dict
    out = {"x": x.numpy(), "gt": gt, "pc_range": np.asarray(RANGE16, np.float32), "keys": keys,
           "box_cls_labels": fr["box_cls_labels"].numpy(), "box_reg_targets": fr["box_reg_targets"].numpy(),
           "batch_box_preds": d["batch_box_preds"].detach().numpy(), "loss": np.float32(loss.item()),
           "loss_cls": np.float32(tb["rpn_loss_cls"]), "loss_loc": np.float32(tb["rpn_loss_loc"]), "loss_dir": np.float32(tb["rpn_loss_dir"])}
    for i in range(2):
        out[f"cls_preds{i}"] = fr["cls_preds"][i].detach().numpy()
        out[f"box_preds{i}"] = fr["box_preds"][i].detach().numpy()
        out[f"dir_preds{i}"] = fr["dir_cls_preds"][i].detach().numpy()
        out[f"batch_cls_preds{i}"] = d["batch_cls_preds"][i].detach().numpy()
        out[f"label_mapping{i}"] = d["multihead_label_mapping"][i].numpy()
    np.savez_compressed(os.path.join(OUT, "anchor_multi_head.npz"), **out, **w)
    print("head", len(keys), "keys, positives", int((fr["box_cls_labels"] > 0).sum()), "loss", float(loss), tb)


def cap_nms(L):
    """Two heads (labels [2] and [1, 3]) over 40 + 60 boxes per sample, batch 2, raw logits.  The boxes are clusters of
    near-duplicates (BEV IoU far above the threshold) on an 8 m lattice (IoU 0 between clusters), so no NMS decision sits
    near NMS_THRESH; one class exceeds NMS_PRE_MAXSIZE candidates and NMS_POST_MAXSIZE survivors."""
    rng = np.random.default_rng(31)
    n0, n1 = 40, 60
    boxes = np.zeros((2, n0 + n1, 9), np.float32)
    for b in range(2):
        for i in range(n0 + n1):
            cluster = i // 4 if i < n0 else (i - n0) // 5
            cx, cy = 8.0 * (cluster % 5), 8.0 * (cluster // 5) + (0 if i < n0 else 40.0)
            boxes[b, i, :7] = [cx + rng.uniform(-0.1, 0.1), cy + rng.uniform(-0.1, 0.1), rng.uniform(-1, 0), 4.0 + rng.uniform(-0.1, 0.1),
                               1.8 + rng.uniform(-0.05, 0.05), 1.5, 0.3 * cluster + rng.uniform(-0.03, 0.03)]
            boxes[b, i, 7:] = rng.uniform(-3, 3, 2)
    cls0 = rng.normal(0.5, 1.5, (2, n0, 1)).astype(np.float32)
    cls1 = rng.normal(-0.3, 1.5, (2, n1, 2)).astype(np.float32)
    cls1[1, :, 1] = -4.0                           # a class with nothing above the score threshold in sample 1

    class Stub(L["detector3d_template"].Detector3DTemplate):
        def __init__(self):
            torch.nn.Module.__init__(self)
            self.num_class = 3
            self.model_cfg = ED(POST_PROCESSING=cases.NMS_CFG)

    batch = {"batch_size": 2, "batch_box_preds": torch.from_numpy(boxes), "batch_cls_preds": [torch.from_numpy(cls0), torch.from_numpy(cls1)],
             "cls_preds_normalized": False, "multihead_label_mapping": [torch.tensor([2]), torch.tensor([1, 3])]}
    preds, _ = Stub().post_processing(batch)
    out = {"boxes": boxes, "cls0": cls0, "cls1": cls1, "mapping0": np.array([2]), "mapping1": np.array([1, 3])}
    for b, p in enumerate(preds):
        out[f"pred_boxes{b}"], out[f"pred_scores{b}"], out[f"pred_labels{b}"] = (p[k].numpy() for k in ("pred_boxes", "pred_scores", "pred_labels"))
        print("nms sample", b, "labels", p["pred_labels"].tolist())
    # the per-class routine alone, on the second head's sigmoid scores of sample 0
    s, l, bx = L["model_nms_utils"].multi_classes_nms(torch.sigmoid(torch.from_numpy(cls1[0])), torch.from_numpy(boxes[0, n0:]),
                                                      ED(cases.NMS_CFG["NMS_CONFIG"]), score_thresh=cases.NMS_CFG["SCORE_THRESH"])
    out["mc_scores"], out["mc_labels"], out["mc_boxes"] = s.numpy(), l.numpy(), bx.numpy()
    # WeightedL1Loss (loss_utils.py) with code weights, nan targets and anchor weights
    a = torch.from_numpy(rng.standard_normal((2, 30, 10)).astype(np.float32))
    t = torch.from_numpy(rng.standard_normal((2, 30, 10)).astype(np.float32))
    t[0, 3, 2] = float("nan")
    w = torch.from_numpy(rng.uniform(0, 1, (2, 30)).astype(np.float32))
    cw = [1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 0.2, 0.2]
    l1 = L["loss_utils"].WeightedL1Loss(code_weights=cw)(a, t, w)
    out.update(l1_a=a.numpy(), l1_t=t.numpy(), l1_w=w.numpy(), l1_code_weights=np.asarray(cw, np.float32), l1=l1.numpy())
    np.savez_compressed(os.path.join(OUT, "anchor_multi_nms.npz"), **out)


def main():
    L = setup()
    cap_assign(L)
    cap_head(L)
    cap_nms(L)
    for f in ("anchor_multi_assign.npz", "anchor_multi_head.npz", "anchor_multi_nms.npz"):
        print(f, os.path.getsize(os.path.join(OUT, f)) // 1024, "KiB")


if __name__ == "__main__":
    main()
