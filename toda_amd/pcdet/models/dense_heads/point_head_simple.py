"""PointHeadSimple (reference pcdet/models/dense_heads/point_head_simple.py:6-91): PV-RCNN's keypoint segmentation head.
Writes point_cls_scores, which PVRCNNHead uses to weight the keypoint features."""
import torch

from ...utils import box_utils
from .point_head_template import PointHeadTemplate


class PointHeadSimple(PointHeadTemplate):
    def __init__(self, num_class, input_channels, model_cfg, **kwargs):
        super().__init__(model_cfg=model_cfg, num_class=num_class)
        self.cls_layers = self.make_fc_layers(fc_cfg=model_cfg.CLS_FC, input_channels=input_channels, output_channels=num_class)

    def assign_targets(self, input_dict):
        point_coords = input_dict["point_coords"]
        gt_boxes = input_dict["gt_boxes"]
        assert gt_boxes.dim() == 3, f"gt_boxes.shape={tuple(gt_boxes.shape)}"
        assert point_coords.dim() == 2, f"points.shape={tuple(point_coords.shape)}"
        batch_size = gt_boxes.shape[0]
        extend_gt_boxes = box_utils.enlarge_box3d(gt_boxes.view(-1, gt_boxes.shape[-1]),
                                                  extra_width=self.model_cfg.TARGET_CONFIG.GT_EXTRA_WIDTH).view(batch_size, -1, gt_boxes.shape[-1])
        return self.assign_stack_targets(points=point_coords, gt_boxes=gt_boxes, extend_gt_boxes=extend_gt_boxes, set_ignore_flag=True,
                                         use_ball_constraint=False, ret_part_labels=False)

    def get_loss(self, tb_dict=None):
        tb_dict = {} if tb_dict is None else tb_dict
        point_loss_cls, tb_dict_1 = self.get_cls_layer_loss()
        tb_dict.update(tb_dict_1)
        return point_loss_cls, tb_dict

    def forward(self, batch_dict):
        if self.model_cfg.get("USE_POINT_FEATURES_BEFORE_FUSION", False):
            point_features = batch_dict["point_features_before_fusion"]
        else:
            point_features = batch_dict["point_features"]
        point_cls_preds = self.run_fc(self.cls_layers, point_features)
        ret_dict = {"point_cls_preds": point_cls_preds}
        point_cls_scores = torch.sigmoid(point_cls_preds)
        batch_dict["point_cls_scores"], _ = point_cls_scores.max(dim=-1)
        if self.training:
            ret_dict["point_cls_labels"] = self.assign_targets(batch_dict)["point_cls_labels"]
        self.forward_ret_dict = ret_dict
        return batch_dict
