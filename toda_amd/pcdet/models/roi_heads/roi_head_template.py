"""RoIHeadTemplate (reference pcdet/models/roi_heads/roi_head_template.py:11-261): proposal layer (top rois of the dense
head after rotated NMS), target assignment (ProposalTargetLayer + canonical transform and heading flip) and the fc-layer
builder whose Conv1d / BatchNorm1d / Dropout keys the checkpoints carry."""
import numpy as np
import torch
import torch.nn as nn

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
