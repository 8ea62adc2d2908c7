"""Inputs of the anchor-assigner tests: small anchor heads, gt boxes drawn next to anchors, and the screening that keeps a
comparison between two fp32 evaluations meaningful.  A gt set is used only when (1) no anchor's best IoU lies within 1e-4 of
a threshold and (2) each gt's set of maximal anchors is the same with the IoU matrix in float64 and in float32; a set that
fails is redrawn from the next seed, never masked."""
import os

import numpy as np
import torch

from toda_amd.pcdet.config import AttrDict

KITTI3 = [("Car", [3.9, 1.6, 1.56], -1.78, 0.6, 0.45), ("Pedestrian", [0.8, 0.6, 1.73], -0.6, 0.5, 0.35),
          ("Cyclist", [1.76, 0.6, 1.73], -0.6, 0.5, 0.35)]
# four classes, the last with a square footprint: both rotations of a square anchor tie exactly
SMALL4 = KITTI3 + [("Cone", [0.8, 0.8, 1.0], -1.0, 0.6, 0.4)]
NUSC10 = [("car", [4.63, 1.97, 1.74], -0.95, 0.6, 0.45), ("truck", [6.93, 2.51, 2.84], -0.6, 0.55, 0.4),
          ("construction_vehicle", [6.37, 2.85, 3.19], -0.225, 0.5, 0.35), ("bus", [10.5, 2.94, 3.47], -0.085, 0.55, 0.4),
          ("trailer", [12.29, 2.90, 3.87], 0.115, 0.5, 0.35), ("barrier", [0.50, 2.53, 0.98], -1.33, 0.55, 0.4),
          ("motorcycle", [2.11, 0.77, 1.47], -1.085, 0.5, 0.3), ("bicycle", [1.70, 0.60, 1.28], -1.18, 0.5, 0.35),
          ("pedestrian", [0.73, 0.67, 1.77], -0.935, 0.6, 0.4), ("traffic_cone", [0.41, 0.41, 1.07], -1.285, 0.6, 0.4)]


def head_cfg(specs, multihead, code_size=7, sincos=False, stride=1):
    gen = [dict(class_name=n, anchor_sizes=[s], anchor_rotations=[0, 1.57], anchor_bottom_heights=[z], align_center=False,
                feature_map_stride=stride, matched_threshold=m, unmatched_threshold=u) for n, s, z, m, u in specs]
    return AttrDict(dict(
        USE_MULTIHEAD=multihead, ANCHOR_GENERATOR_CONFIG=gen,
        TARGET_ASSIGNER_CONFIG=dict(NAME="AxisAlignedTargetAssigner", POS_FRACTION=-1.0, SAMPLE_SIZE=512, NORM_BY_NUM_EXAMPLES=False,
                                    MATCH_HEIGHT=False, BOX_CODER="ResidualCoder",
                                    BOX_CODER_CONFIG=dict(code_size=code_size, encode_angle_by_sincos=sincos))))


# The tiny two-head AnchorHeadMulti of tests/golden/anchor_multi_head.npz and the post-processing settings of
# anchor_multi_nms.npz; tests/golden/capture_anchor_multi.py builds the reference's modules from the same dictionaries.
HEAD_SPECS = KITTI3
HEAD_CFG = dict(
    CLASS_AGNOSTIC=False, USE_DIRECTION_CLASSIFIER=True, DIR_OFFSET=0.78539, DIR_LIMIT_OFFSET=0.0, NUM_DIR_BINS=2,
    USE_MULTIHEAD=True, SEPARATE_MULTIHEAD=True, SHARED_CONV_NUM_FILTER=16,
    RPN_HEAD_CFGS=[dict(HEAD_CLS_NAME=["Car"]), dict(HEAD_CLS_NAME=["Pedestrian", "Cyclist"])],
    SEPARATE_REG_CONFIG=dict(NUM_MIDDLE_CONV=1, NUM_MIDDLE_FILTER=16, REG_LIST=["reg:2", "height:1", "size:3", "angle:1"]),
    LOSS_CONFIG=dict(LOSS_WEIGHTS=dict(pos_cls_weight=1.0, neg_cls_weight=2.0, cls_weight=1.0, loc_weight=0.25, dir_weight=0.2,
                                       code_weights=[1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 0.5])))


def head_model_cfg():
    base = head_cfg(HEAD_SPECS, True)
    return {**HEAD_CFG, "ANCHOR_GENERATOR_CONFIG": list(base["ANCHOR_GENERATOR_CONFIG"]),
            "TARGET_ASSIGNER_CONFIG": dict(base["TARGET_ASSIGNER_CONFIG"])}


NMS_CFG = dict(RECALL_THRESH_LIST=[0.3, 0.5], SCORE_THRESH=0.3, OUTPUT_RAW_SCORE=False,
               NMS_CONFIG=dict(MULTI_CLASSES_NMS=True, NMS_TYPE="nms_gpu", NMS_THRESH=0.2, NMS_PRE_MAXSIZE=30, NMS_POST_MAXSIZE=6))


def make_assigner(specs, grid_xy, pc_range, multihead, code_size=7, sincos=False, class_names=None):
    """(assigner, per-class anchor tables on the CPU) for a grid_xy = (nx, ny) map, built the way AnchorHeadTemplate does."""
    from toda_amd.pcdet.models.dense_heads.anchor_head_template import AnchorHeadTemplate
    from toda_amd.pcdet.models.dense_heads.target_assigner.axis_aligned_target_assigner import AxisAlignedTargetAssigner
    from toda_amd.pcdet.utils import box_coder_utils

    cfg = head_cfg(specs, multihead, code_size, sincos)
    coder = box_coder_utils.ResidualCoder(code_size=code_size, encode_angle_by_sincos=sincos)
    anchors, _ = AnchorHeadTemplate.generate_anchors(cfg.ANCHOR_GENERATOR_CONFIG, grid_size=np.array([grid_xy[0], grid_xy[1], 1]),
                                                     point_cloud_range=np.asarray(pc_range, np.float32), anchor_ndim=coder.code_size)
    names = class_names or [s[0] for s in specs]
    return AxisAlignedTargetAssigner(cfg, names, coder, match_height=False), anchors


def draw_gt(seed, specs, pc_range, batch, n_gt, n_extra=0, counts=None, class_pool=None):
    """[batch, n_gt, 7 + n_extra + 1] fp32: per sample counts[b] boxes (default: all n_gt) whose sizes sit near their
    class's anchor and whose headings cluster around the two anchor rotations, then zero padding."""
    rng = np.random.default_rng(seed)
    gt = np.zeros((batch, n_gt, 8 + n_extra), np.float32)
    pool = class_pool if class_pool is not None else list(range(len(specs)))
    for b in range(batch):
        for m in range(n_gt if counts is None else counts[b]):
            c = pool[int(rng.integers(0, len(pool)))]
            size = np.asarray(specs[c][1]) * rng.uniform(0.85, 1.15, 3)
            x = rng.uniform(pc_range[0] + 1, pc_range[3] - 1)
            y = rng.uniform(pc_range[1] + 1, pc_range[4] - 1)
            yaw = [0.0, np.pi / 2, -np.pi / 2, np.pi][int(rng.integers(0, 4))] + rng.uniform(-0.3, 0.3)
            gt[b, m, :7] = [x, y, specs[c][2] + size[2] / 2, *size, yaw]
            gt[b, m, 7:7 + n_extra] = rng.uniform(-3, 3, n_extra)
            gt[b, m, -1] = c + 1
    return gt


def aligned_rect(boxes, dtype):
    b = boxes.astype(dtype)
    pi = dtype(np.pi)
    rot = np.abs(b[:, 6] - np.floor(b[:, 6] / pi + dtype(0.5)) * pi)
    keep = (rot < dtype(np.pi / 4))[:, None]
    dims = np.where(keep, b[:, [3, 4]], b[:, [4, 3]])
    return np.concatenate([b[:, 0:2] - dims / dtype(2), b[:, 0:2] + dims / dtype(2)], 1)


def iou_matrix(anchors, gts, dtype):
    """box_utils.boxes3d_nearest_bev_iou in numpy at `dtype`, the same operation order."""
    a, g = aligned_rect(anchors, dtype), aligned_rect(gts, dtype)
    lo = np.maximum(a[:, None, 0:2], g[None, :, 0:2])
    hi = np.minimum(a[:, None, 2:4], g[None, :, 2:4])
    wh = np.maximum(hi - lo, dtype(0))
    inter = wh[..., 0] * wh[..., 1]
    area_a = (a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1])
    area_g = (g[:, 2] - g[:, 0]) * (g[:, 3] - g[:, 1])
    return inter / np.maximum(area_a[:, None] + area_g[None, :] - inter, dtype(1e-6))


def screening_failures(anchors, gt, specs, class_names=None):
    """List of (sample, class, reason) where the two screening conditions do not hold; empty = the set is usable."""
    names = class_names or [s[0] for s in specs]
    bad = []
    for b in range(gt.shape[0]):
        for c, (name, _, _, matched, unmatched) in enumerate(specs):
            ids = gt[b, :, -1].astype(np.int64)
            sel = np.array([1 <= i <= len(names) and names[i - 1] == name for i in ids], bool)
            if not sel.any():
                continue
            table = anchors[c].reshape(-1, anchors[c].shape[-1]).numpy()
            i32, i64 = iou_matrix(table, gt[b, sel], np.float32), iou_matrix(table, gt[b, sel], np.float64)
            best = i32.max(1)
            if (np.abs(best - np.float32(matched)) < 1e-4).any() or (np.abs(best - np.float32(unmatched)) < 1e-4).any():
                bad.append((b, c, "threshold"))
            if not np.array_equal(i32 == i32.max(0, keepdims=True), i64 == i64.max(0, keepdims=True)):
                bad.append((b, c, "maximal set"))
    return bad


def first_screened(make, seed, anchors, specs, tries=200):
    """make(seed), make(seed + 1000), ...: the first gt set that passes the screening."""
    for k in range(tries):
        gt = make(seed + 1000 * k)
        if not screening_failures(anchors, gt, specs):
            return gt
    raise AssertionError(f"no screened gt set in {tries} draws")


def screened_gt(seed, anchors, specs, pc_range, batch, n_gt, **kw):
    """The first draw from seed, seed + 1000, ... that passes the screening."""
    return first_screened(lambda s: draw_gt(s, specs, pc_range, batch, n_gt, **kw), seed, anchors, specs)


def encode_f64(gt_rows, anchor_rows, sincos):
    """ResidualCoder.encode_torch in float64 from the fp32 inputs (sizes clamped at fp32 1e-5 first)."""
    g, a = gt_rows.astype(np.float64), anchor_rows.astype(np.float64)
    lo = float(np.float32(1e-5))
    g[:, 3:6], a[:, 3:6] = np.maximum(g[:, 3:6], lo), np.maximum(a[:, 3:6], lo)
    diag = np.sqrt(a[:, 3] ** 2 + a[:, 4] ** 2)
    cols = [(g[:, 0] - a[:, 0]) / diag, (g[:, 1] - a[:, 1]) / diag, (g[:, 2] - a[:, 2]) / a[:, 5],
            np.log(g[:, 3] / a[:, 3]), np.log(g[:, 4] / a[:, 4]), np.log(g[:, 5] / a[:, 5])]
    cols += [np.cos(g[:, 6]) - np.cos(a[:, 6]), np.sin(g[:, 6]) - np.sin(a[:, 6])] if sincos else [g[:, 6] - a[:, 6]]
    n_extra = min(g.shape[1], a.shape[1]) - 7
    cols += [g[:, 7 + i] - a[:, 7 + i] for i in range(n_extra)]
    return np.stack(cols, 1)


def flat_anchors(anchors, multihead):
    if multihead:
        return torch.cat([t.permute(3, 4, 0, 1, 2, 5).contiguous().view(-1, t.shape[-1]) for t in anchors], 0)
    return torch.cat(anchors, dim=-3).view(-1, anchors[0].shape[-1])


# ---------------------------------------------------------------- checks against the reference-captured fixtures
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
RANGE16 = [0.0, -8.0, -3.0, 16.0, 8.0, 1.0]
ASSIGN_CASES = [("c7", 7, False), ("c9", 9, True)]


def load(name):
    with np.load(os.path.join(GOLDEN, f"{name}.npz"), allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def fixture_anchors(g, tag):
    return [torch.from_numpy(g[f"{tag}_anchors{k}"]) for k in range(len(SMALL4))]


def check_assign_fixture(route, device):
    """AxisAlignedTargetAssigner (route "torch" or "hip") on the inputs of anchor_multi_assign.npz against the reference's
    labels, weights and targets, both anchor orders, code size 7 and 9 + sin/cos.  Targets at the tolerance the C1 chain test
    uses for them (rtol 1e-5, atol 1e-6)."""
    g = load("anchor_multi_assign")
    for tag, code_size, sincos in ASSIGN_CASES:
        for multihead in (False, True):
            assigner, mine = make_assigner(SMALL4, (16, 16), RANGE16, multihead, code_size, sincos)
            anchors = fixture_anchors(g, tag)
            for a, b in zip(mine, anchors):
                np.testing.assert_allclose(a.numpy(), b.numpy(), rtol=0, atol=1e-6)
            anchors = [a.to(device) for a in anchors]
            gt = torch.from_numpy(g[f"{tag}_gt"].copy()).to(device)
            out = getattr(assigner, f"assign_targets_{route}")(anchors, gt)
            order = "multi" if multihead else "single"
            labels = out["box_cls_labels"].cpu().numpy()
            assert (labels > 0).sum() > 0
            assert np.array_equal(labels, g[f"{tag}_{order}_labels"]), (tag, order)
            np.testing.assert_allclose(out["reg_weights"].cpu().numpy(), g[f"{tag}_{order}_weights"], rtol=0, atol=0)
            targets = out["box_reg_targets"].cpu().numpy()
            err = np.abs(targets - g[f"{tag}_{order}_targets"]).max()
            print(f"{route} {tag} {order}: positives {int((labels > 0).sum())}, max |target - reference| {err:.3e}")
            np.testing.assert_allclose(targets, g[f"{tag}_{order}_targets"], rtol=1e-5, atol=1e-6)
            assert not targets[labels <= 0].view(np.uint32).any()


def check_head_fixture(device, tol=1.0):
    """The port's AnchorHeadMulti with the reference's weights on the input map of anchor_multi_head.npz: parameter keys,
    per-head predictions, targets, decoded boxes, label mapping and the class / box / direction losses, at the tolerances
    of the C1 chain check (predictions rtol 1e-4 atol 1e-5, losses 1e-4 relative, each times tol)."""
    from toda_amd.pcdet.models.dense_heads import AnchorHeadMulti

    g = load("anchor_multi_head")
    names = [s[0] for s in HEAD_SPECS]
    head = AnchorHeadMulti(AttrDict(head_model_cfg()), 24, 3, names, np.array([16, 16, 1]), g["pc_range"],
                           predict_boxes_when_training=True).train()
    assert list(head.state_dict()) == [str(k) for k in g["keys"]]
    head.load_state_dict({k[2:]: torch.from_numpy(v) for k, v in g.items() if k.startswith("w.")}, strict=True)
    head = head.to(device)
    head.anchors = [a.to(device) for a in head.anchors]
    d = head({"spatial_features_2d": torch.from_numpy(g["x"]).to(device), "gt_boxes": torch.from_numpy(g["gt"].copy()).to(device),
              "batch_size": 2})
    fr = head.forward_ret_dict

    def close(mine, ref, what):
        mine = mine.detach().cpu().numpy()
        print(f"{what}: max |port - reference| {np.abs(mine - g[ref]).max():.3e}")
        np.testing.assert_allclose(mine, g[ref], rtol=1e-4 * tol, atol=1e-5 * tol, err_msg=what)

    for i in range(2):
        close(fr["cls_preds"][i], f"cls_preds{i}", f"cls_preds[{i}]")
        close(fr["box_preds"][i], f"box_preds{i}", f"box_preds[{i}]")
        close(fr["dir_cls_preds"][i], f"dir_preds{i}", f"dir_cls_preds[{i}]")
        close(d["batch_cls_preds"][i], f"batch_cls_preds{i}", f"batch_cls_preds[{i}]")
        assert d["multihead_label_mapping"][i].tolist() == g[f"label_mapping{i}"].tolist()
    assert np.array_equal(fr["box_cls_labels"].cpu().numpy(), g["box_cls_labels"])
    np.testing.assert_allclose(fr["box_reg_targets"].cpu().numpy(), g["box_reg_targets"], rtol=1e-5, atol=1e-6)
    close(d["batch_box_preds"], "batch_box_preds", "decoded boxes")
    loss, tb = head.get_loss()
    for mine, ref in ((loss, "loss"), (tb["rpn_loss_cls"], "loss_cls"), (tb["rpn_loss_loc"], "loss_loc"), (tb["rpn_loss_dir"], "loss_dir")):
        print(f"{ref}: port {float(mine.detach()):.7f} reference {float(g[ref]):.7f}")
        assert abs(float(mine.detach()) - float(g[ref])) < 1e-4 * tol * max(1.0, abs(float(g[ref]))), ref


def check_nms_fixture(device):
    """Detector3DTemplate.post_processing (MULTI_CLASSES_NMS over two heads' score lists) and multi_classes_nms alone on the
    inputs of anchor_multi_nms.npz: the same rows in the same order as the reference's."""
    from toda_amd.pcdet.models.detectors.detector3d_template import Detector3DTemplate
    from toda_amd.pcdet.models.model_utils import model_nms_utils

    g = load("anchor_multi_nms")

    class Stub(Detector3DTemplate):
        def __init__(self):
            torch.nn.Module.__init__(self)
            self.num_class = 3
            self.model_cfg = AttrDict(dict(POST_PROCESSING=NMS_CFG))

    T = lambda a: torch.from_numpy(a).to(device)  # noqa: E731
    batch = {"batch_size": 2, "batch_box_preds": T(g["boxes"]), "batch_cls_preds": [T(g["cls0"]), T(g["cls1"])],
             "cls_preds_normalized": False, "multihead_label_mapping": [T(g["mapping0"]), T(g["mapping1"])]}
    preds, _ = Stub().post_processing(batch)
    for b, p in enumerate(preds):
        assert p["pred_labels"].cpu().tolist() == g[f"pred_labels{b}"].tolist(), b
        np.testing.assert_allclose(p["pred_scores"].cpu().numpy(), g[f"pred_scores{b}"], rtol=1e-6, atol=1e-7)
        assert np.array_equal(p["pred_boxes"].cpu().numpy(), g[f"pred_boxes{b}"]), b
    n0 = g["cls0"].shape[1]
    s, l, bx = model_nms_utils.multi_classes_nms(torch.sigmoid(T(g["cls1"][0])), T(g["boxes"][0, n0:]),
                                                 AttrDict(NMS_CFG["NMS_CONFIG"]), score_thresh=NMS_CFG["SCORE_THRESH"])
    assert l.dtype == torch.long and l.cpu().tolist() == g["mc_labels"].tolist()
    np.testing.assert_allclose(s.cpu().numpy(), g["mc_scores"], rtol=1e-6, atol=1e-7)
    assert np.array_equal(bx.cpu().numpy(), g["mc_boxes"])
