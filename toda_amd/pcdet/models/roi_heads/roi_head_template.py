"""RoIHeadTemplate (reference pcdet/models/roi_heads/roi_head_template.py:11-261): proposal layer (top rois of the dense
head after rotated NMS), target assignment (ProposalTargetLayer + canonical transform and heading flip) and the fc-layer
builder whose Conv1d / BatchNorm1d / Dropout keys the checkpoints carry."""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from ...utils import box_coder_utils, common_utils, loss_utils
from ..model_utils.model_nms_utils import class_agnostic_nms
from .target_assigner.proposal_target_layer import ProposalTargetLayer


class RoIHeadTemplate(nn.Module):
    def __init__(self, num_class, model_cfg, **kwargs):
        super().__init__()
        self.model_cfg = model_cfg
        self.num_class = num_class
        self.box_coder = getattr(box_coder_utils, model_cfg.TARGET_CONFIG.BOX_CODER)(
            **model_cfg.TARGET_CONFIG.get("BOX_CODER_CONFIG", {}))
        self.proposal_target_layer = ProposalTargetLayer(roi_sampler_cfg=model_cfg.TARGET_CONFIG)
        self.build_losses(model_cfg.LOSS_CONFIG)
        self.forward_ret_dict = None

    def build_losses(self, losses_cfg):
        self.add_module("reg_loss_func", loss_utils.WeightedSmoothL1Loss(code_weights=losses_cfg.LOSS_WEIGHTS["code_weights"]))

    def make_fc_layers(self, input_channels, output_channels, fc_list):
        """[Conv1d(k=1, no bias), BatchNorm1d, ReLU] per entry, Dropout(DP_RATIO) after the first one when DP_RATIO >= 0, then a
        Conv1d with bias to output_channels."""
        layers, pre = [], input_channels
        for k, width in enumerate(fc_list):
            layers += [nn.Conv1d(pre, width, kernel_size=1, bias=False), nn.BatchNorm1d(width), nn.ReLU()]
            pre = width
            if self.model_cfg.DP_RATIO >= 0 and k == 0:
                layers.append(nn.Dropout(self.model_cfg.DP_RATIO))
        layers.append(nn.Conv1d(pre, output_channels, kernel_size=1, bias=True))
        return nn.Sequential(*layers)

    @torch.no_grad()
    def proposal_layer(self, batch_dict, nms_config):
        """batch_cls_preds [B, A, K] / batch_box_preds [B, A, 7 + C] of the dense head -> rois [B, NMS_POST_MAXSIZE, 7 + C],
        roi_scores, roi_labels (1-based), zero rows where NMS kept fewer boxes."""
        if batch_dict.get("rois", None) is not None:
            return batch_dict
        batch_size = batch_dict["batch_size"]
        box_preds_all, cls_preds_all = batch_dict["batch_box_preds"], batch_dict["batch_cls_preds"]
        n_post = nms_config.NMS_POST_MAXSIZE
        rois = box_preds_all.new_zeros((batch_size, n_post, box_preds_all.shape[-1]))
        roi_scores = box_preds_all.new_zeros((batch_size, n_post))
        roi_labels = box_preds_all.new_zeros((batch_size, n_post), dtype=torch.long)
        for index in range(batch_size):
            if batch_dict.get("batch_index", None) is not None:
                assert cls_preds_all.dim() == 2
                pick = batch_dict["batch_index"] == index
            else:
                assert cls_preds_all.dim() == 3
                pick = index
            box_preds, cls_preds = box_preds_all[pick], cls_preds_all[pick]
            scores, labels = torch.max(cls_preds, dim=1)
            if nms_config.MULTI_CLASSES_NMS:
                raise NotImplementedError("MULTI_CLASSES_NMS proposals")
            selected, _ = class_agnostic_nms(box_scores=scores, box_preds=box_preds, nms_config=nms_config)
            n = selected.shape[0]
            rois[index, :n] = box_preds[selected]
            roi_scores[index, :n] = scores[selected]
            roi_labels[index, :n] = labels[selected]
        batch_dict["rois"] = rois
        batch_dict["roi_scores"] = roi_scores
        batch_dict["roi_labels"] = roi_labels + 1
        batch_dict["has_class_labels"] = cls_preds_all.shape[-1] > 1
        batch_dict.pop("batch_index", None)
        return batch_dict

    def assign_targets(self, batch_dict):
        """Sampled rois and their gts; gt_of_rois in the roi's frame (centre at the origin, heading relative to the roi's,
        flipped into (-pi/2, pi/2))."""
        batch_size = batch_dict["batch_size"]
        with torch.no_grad():
            targets_dict = self.proposal_target_layer.forward(batch_dict)
        rois, gt_of_rois = targets_dict["rois"], targets_dict["gt_of_rois"]
        targets_dict["gt_of_rois_src"] = gt_of_rois.clone().detach()

        roi_ry = rois[:, :, 6] % (2 * np.pi)
        gt_of_rois[:, :, 0:3] = gt_of_rois[:, :, 0:3] - rois[:, :, 0:3]
        gt_of_rois[:, :, 6] = gt_of_rois[:, :, 6] - roi_ry
        gt_of_rois = common_utils.rotate_points_along_z(points=gt_of_rois.view(-1, 1, gt_of_rois.shape[-1]),
                                                        angle=-roi_ry.view(-1)).view(batch_size, -1, gt_of_rois.shape[-1])
        heading = gt_of_rois[:, :, 6] % (2 * np.pi)
        opposite = (heading > np.pi * 0.5) & (heading < np.pi * 1.5)
        heading = torch.where(opposite, (heading + np.pi) % (2 * np.pi), heading)
        heading = torch.where(heading > np.pi, heading - np.pi * 2, heading)
        gt_of_rois[:, :, 6] = torch.clamp(heading, min=-np.pi / 2, max=np.pi / 2)
        targets_dict["gt_of_rois"] = gt_of_rois
        return targets_dict

    def get_box_reg_layer_loss(self, forward_ret_dict):
        """Smooth-L1 of the residual-coded box in the roi's frame over the foreground rois, plus the corner regularisation of the
        decoded box against the gt in the lidar frame (reference roi_head_template.py:136-196)."""
        loss_cfgs = self.model_cfg.LOSS_CONFIG
        code_size = self.box_coder.code_size
        reg_valid_mask = forward_ret_dict["reg_valid_mask"].view(-1)
        gt_boxes3d_ct = forward_ret_dict["gt_of_rois"][..., 0:code_size]
        gt_of_rois_src = forward_ret_dict["gt_of_rois_src"][..., 0:code_size].view(-1, code_size)
        rcnn_reg = forward_ret_dict["rcnn_reg"]
        roi_boxes3d = forward_ret_dict["rois"]
        rcnn_batch_size = gt_boxes3d_ct.view(-1, code_size).shape[0]
        fg_mask = reg_valid_mask > 0
        fg_sum = int(fg_mask.long().sum().item())
        tb_dict = {}
        if loss_cfgs.REG_LOSS != "smooth-l1":
            raise NotImplementedError(f"REG_LOSS {loss_cfgs.REG_LOSS}")
        rois_anchor = roi_boxes3d.clone().detach().view(-1, code_size)
        rois_anchor[:, 0:3] = 0
        rois_anchor[:, 6] = 0
        reg_targets = self.box_coder.encode_torch(gt_boxes3d_ct.view(rcnn_batch_size, code_size), rois_anchor)
        rcnn_loss_reg = self.reg_loss_func(rcnn_reg.view(rcnn_batch_size, -1).unsqueeze(dim=0), reg_targets.unsqueeze(dim=0))
        rcnn_loss_reg = (rcnn_loss_reg.view(rcnn_batch_size, -1) * fg_mask.unsqueeze(dim=-1).float()).sum() / max(fg_sum, 1)
        rcnn_loss_reg = rcnn_loss_reg * loss_cfgs.LOSS_WEIGHTS["rcnn_reg_weight"]
        tb_dict["rcnn_loss_reg"] = rcnn_loss_reg.detach()
        if loss_cfgs.CORNER_LOSS_REGULARIZATION and fg_sum > 0:
            fg_rcnn_reg = rcnn_reg.view(rcnn_batch_size, -1)[fg_mask]
            fg_roi_boxes3d = roi_boxes3d.view(-1, code_size)[fg_mask].view(1, -1, code_size)
            batch_anchors = fg_roi_boxes3d.clone().detach()
            roi_ry = fg_roi_boxes3d[:, :, 6].view(-1)
            roi_xyz = fg_roi_boxes3d[:, :, 0:3].view(-1, 3)
            batch_anchors[:, :, 0:3] = 0
            rcnn_boxes3d = self.box_coder.decode_torch(fg_rcnn_reg.view(batch_anchors.shape[0], -1, code_size), batch_anchors).view(-1, code_size)
            rcnn_boxes3d = common_utils.rotate_points_along_z(rcnn_boxes3d.unsqueeze(dim=1), roi_ry).squeeze(dim=1)
            rcnn_boxes3d[:, 0:3] += roi_xyz
            loss_corner = loss_utils.get_corner_loss_lidar(rcnn_boxes3d[:, 0:7], gt_of_rois_src[fg_mask][:, 0:7]).mean()
            loss_corner = loss_corner * loss_cfgs.LOSS_WEIGHTS["rcnn_corner_weight"]
            rcnn_loss_reg = rcnn_loss_reg + loss_corner
            tb_dict["rcnn_loss_corner"] = loss_corner.detach()
        return rcnn_loss_reg, tb_dict

    def get_box_cls_layer_loss(self, forward_ret_dict):
        """BinaryCrossEntropy on sigmoid(rcnn_cls) or CrossEntropy, averaged over the rois with a label >= 0 (reference
        roi_head_template.py:198-216)."""
        loss_cfgs = self.model_cfg.LOSS_CONFIG
        rcnn_cls = forward_ret_dict["rcnn_cls"]
        rcnn_cls_labels = forward_ret_dict["rcnn_cls_labels"].view(-1)
        if loss_cfgs.CLS_LOSS == "BinaryCrossEntropy":
            batch_loss_cls = F.binary_cross_entropy(torch.sigmoid(rcnn_cls.view(-1)), rcnn_cls_labels.float(), reduction="none")
        elif loss_cfgs.CLS_LOSS == "CrossEntropy":
            batch_loss_cls = F.cross_entropy(rcnn_cls, rcnn_cls_labels, reduction="none", ignore_index=-1)
        else:
            raise NotImplementedError(f"CLS_LOSS {loss_cfgs.CLS_LOSS}")
        cls_valid_mask = (rcnn_cls_labels >= 0).float()
        rcnn_loss_cls = (batch_loss_cls * cls_valid_mask).sum() / torch.clamp(cls_valid_mask.sum(), min=1.0)
        rcnn_loss_cls = rcnn_loss_cls * loss_cfgs.LOSS_WEIGHTS["rcnn_cls_weight"]
        return rcnn_loss_cls, {"rcnn_loss_cls": rcnn_loss_cls.detach()}

    def get_loss(self, tb_dict=None):
        """Classification + box regression losses of the refined rois (reference roi_head_template.py:218-229)."""
        tb_dict = {} if tb_dict is None else tb_dict
        rcnn_loss_cls, cls_tb_dict = self.get_box_cls_layer_loss(self.forward_ret_dict)
        tb_dict.update(cls_tb_dict)
        rcnn_loss_reg, reg_tb_dict = self.get_box_reg_layer_loss(self.forward_ret_dict)
        tb_dict.update(reg_tb_dict)
        rcnn_loss = rcnn_loss_cls + rcnn_loss_reg
        tb_dict["rcnn_loss"] = rcnn_loss.detach()
        return rcnn_loss, tb_dict

    def generate_predicted_boxes(self, batch_size, rois, cls_preds, box_preds):
        """Decode box_preds [B * N, code] relative to the rois (local frame, then rotated and shifted back)."""
        code_size = self.box_coder.code_size
        batch_cls_preds = cls_preds.view(batch_size, -1, cls_preds.shape[-1])
        batch_box_preds = box_preds.view(batch_size, -1, code_size)
        roi_ry, roi_xyz = rois[:, :, 6].view(-1), rois[:, :, 0:3].view(-1, 3)
        local_rois = rois.clone().detach()
        local_rois[:, :, 0:3] = 0
        batch_box_preds = self.box_coder.decode_torch(batch_box_preds, local_rois).view(-1, code_size)
        batch_box_preds = common_utils.rotate_points_along_z(batch_box_preds.unsqueeze(dim=1), roi_ry).squeeze(dim=1)
        batch_box_preds[:, 0:3] += roi_xyz
        return batch_cls_preds, batch_box_preds.view(batch_size, -1, code_size)
