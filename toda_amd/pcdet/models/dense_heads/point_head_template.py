"""PointHeadTemplate (reference pcdet/models/dense_heads/point_head_template.py:8-210), the parts PointHeadSimple uses: the fc
stack, stack targets from points_in_boxes on the gt boxes and the enlarged gt boxes (ignore band), the sigmoid focal
classification loss."""
import torch
import torch.nn as nn

from ...utils import loss_utils
from ..roi_heads.second_head import run_fc_rows


def points_in_boxes_torch(points, boxes):
    """points [N, 3], boxes [M, 7] (CPU) -> [N] int64 index of the first box holding each point, -1 for none (the test of the
    reference's roiaware_pool3d_kernel.cu check_pt_in_box3d: |z - cz| <= dz / 2, |local x| < dx / 2 + 1e-5, |local y| < dy / 2 +
    1e-5 after rotating by -heading)."""
    n = points.shape[0]
    out = torch.full((n,), -1, dtype=torch.int64)
    for k in range(boxes.shape[0] - 1, -1, -1):
        cx, cy, cz, dx, dy, dz, rz = [boxes[k, i] for i in range(7)]
        cosa, sina = torch.cos(-rz), torch.sin(-rz)
        sx, sy = points[:, 0] - cx, points[:, 1] - cy
        lx = sx * cosa + sy * (-sina)
        ly = sx * sina + sy * cosa
        inside = ((points[:, 2] - cz).abs() <= dz / 2.0) & (lx.abs() < dx / 2.0 + 1e-5) & (ly.abs() < dy / 2.0 + 1e-5)
        out[inside] = k
    return out


def _box_index(points_single, boxes):
    if points_single.is_cuda:
        from ...ops.roiaware_pool3d import roiaware_pool3d_utils
        return roiaware_pool3d_utils.points_in_boxes_gpu(points_single.unsqueeze(0), boxes.unsqueeze(0).contiguous()).long().squeeze(0)
    return points_in_boxes_torch(points_single, boxes)


class PointHeadTemplate(nn.Module):
    def __init__(self, model_cfg, num_class):
        super().__init__()
        self.model_cfg = model_cfg
        self.num_class = num_class
        self.add_module("cls_loss_func", loss_utils.SigmoidFocalClassificationLoss(alpha=0.25, gamma=2.0))
        self.forward_ret_dict = None

    @staticmethod
    def make_fc_layers(fc_cfg, input_channels, output_channels):
        fc_layers = []
        c_in = input_channels
        for k in range(len(fc_cfg)):
            fc_layers.extend([nn.Linear(c_in, fc_cfg[k], bias=False), nn.BatchNorm1d(fc_cfg[k]), nn.ReLU()])
            c_in = fc_cfg[k]
        fc_layers.append(nn.Linear(c_in, output_channels, bias=True))
        return nn.Sequential(*fc_layers)

    @staticmethod
    def run_fc(seq, x):
        """The fc stack on rows: Linear, then BatchNorm1d + ReLU fused on the device where ops.bn_rows covers the width."""
        return run_fc_rows(seq, x)

    def assign_stack_targets(self, points, gt_boxes, extend_gt_boxes=None, ret_box_labels=False, ret_part_labels=False,
                             set_ignore_flag=True, use_ball_constraint=False, central_radius=2.0):
        """points [N1 + N2 + ..., 4] (bs_idx, x, y, z), gt_boxes [B, M, 8] -> point_cls_labels [N] long (0 background, -1 ignored);
        the set_ignore_flag branch of the reference (:77-166), the only one PointHeadSimple takes."""
        assert len(points.shape) == 2 and points.shape[1] == 4, f"points.shape={tuple(points.shape)}"
        assert len(gt_boxes.shape) == 3 and gt_boxes.shape[2] == 8, f"gt_boxes.shape={tuple(gt_boxes.shape)}"
        if ret_box_labels or ret_part_labels or not set_ignore_flag or use_ball_constraint:
            raise NotImplementedError("box / part labels and the ball constraint belong to PointHeadBox / PointRCNN: out of scope")
        batch_size = gt_boxes.shape[0]
        bs_idx = points[:, 0]
        point_cls_labels = points.new_zeros(points.shape[0]).long()
        for k in range(batch_size):
            bs_mask = bs_idx == k
            points_single = points[bs_mask][:, 1:4]
            labels_single = point_cls_labels.new_zeros(int(bs_mask.sum()))
            box_idxs_of_pts = _box_index(points_single, gt_boxes[k, :, 0:7])
            fg_flag = box_idxs_of_pts >= 0
            extend_idxs = _box_index(points_single, extend_gt_boxes[k, :, 0:7])
            ignore_flag = fg_flag ^ (extend_idxs >= 0)
            labels_single[ignore_flag] = -1
            gt_box_of_fg_points = gt_boxes[k][box_idxs_of_pts[fg_flag]]
            labels_single[fg_flag] = 1 if self.num_class == 1 else gt_box_of_fg_points[:, -1].long()
            point_cls_labels[bs_mask] = labels_single
        return {"point_cls_labels": point_cls_labels, "point_box_labels": None, "point_part_labels": None}

    def get_cls_layer_loss(self, tb_dict=None):
        point_cls_labels = self.forward_ret_dict["point_cls_labels"].view(-1)
        point_cls_preds = self.forward_ret_dict["point_cls_preds"].view(-1, self.num_class)
        positives = point_cls_labels > 0
        negative_cls_weights = (point_cls_labels == 0) * 1.0
        cls_weights = (negative_cls_weights + 1.0 * positives).float()
        pos_normalizer = positives.sum(dim=0).float()
        cls_weights /= torch.clamp(pos_normalizer, min=1.0)
        one_hot_targets = point_cls_preds.new_zeros(*list(point_cls_labels.shape), self.num_class + 1)
        one_hot_targets.scatter_(-1, (point_cls_labels * (point_cls_labels >= 0).long()).unsqueeze(dim=-1).long(), 1.0)
        one_hot_targets = one_hot_targets[..., 1:]
        cls_loss_src = self.cls_loss_func(point_cls_preds, one_hot_targets, weights=cls_weights)
        point_loss_cls = cls_loss_src.sum() * self.model_cfg.LOSS_CONFIG.LOSS_WEIGHTS["point_cls_weight"]
        if tb_dict is None:
            tb_dict = {}
        tb_dict.update({"point_loss_cls": point_loss_cls.detach(), "point_pos_num": pos_normalizer.detach()})
        return point_loss_cls, tb_dict
