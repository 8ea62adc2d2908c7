"""ProposalTargetLayer (reference pcdet/models/roi_heads/target_assigner/proposal_target_layer.py:7-228).

The per-roi best 3-D IoU and its gt index come from one launch for the whole batch (ops.roi_iou3d_max, class restriction and
valid-gt count on the device) instead of a per-sample, per-class Python loop with host syncs.  The roi subsampling stays on
the host with the reference's random draws in the reference's order (np.random.permutation, np.random.rand, torch.randint on
the CPU generator), so a seeded run picks the same rois: one D2H of the [B, N] max-IoU table and one H2D of the sampled
indices per step.  Labels, masks and gathers stay on the device."""
import numpy as np
import torch
import torch.nn as nn

from toda_amd import ops


class ProposalTargetLayer(nn.Module):
    def __init__(self, roi_sampler_cfg):
        super().__init__()
        self.roi_sampler_cfg = roi_sampler_cfg

    def forward(self, batch_dict):
        """batch_dict: batch_size, rois [B, N, 7 + C], roi_scores [B, N], roi_labels [B, N], gt_boxes [B, M, 7 + C + 1].
        Returns rois / gt_of_rois / gt_iou_of_rois / roi_scores / roi_labels / reg_valid_mask / rcnn_cls_labels, M = ROI_PER_IMAGE."""
        cfg = self.roi_sampler_cfg
        rois, gt_of_rois, ious, roi_scores, roi_labels = self.sample_rois_for_rcnn(batch_dict)
        reg_valid_mask = (ious > cfg.REG_FG_THRESH).long()
        if cfg.CLS_SCORE_TYPE == "cls":
            cls_labels = (ious > cfg.CLS_FG_THRESH).long()
            ignore = (ious > cfg.CLS_BG_THRESH) & (ious < cfg.CLS_FG_THRESH)
            cls_labels = torch.where(ignore, torch.full_like(cls_labels, -1), cls_labels)
        elif cfg.CLS_SCORE_TYPE == "roi_iou":
            lo, hi = cfg.CLS_BG_THRESH, cfg.CLS_FG_THRESH
            fg, bg = ious > hi, ious < lo
            between = ~fg & ~bg
            cls_labels = torch.where(between, (ious - lo) / (hi - lo), fg.float())
        else:
            raise NotImplementedError(f"CLS_SCORE_TYPE {cfg.CLS_SCORE_TYPE}")
        return {"rois": rois, "gt_of_rois": gt_of_rois, "gt_iou_of_rois": ious, "roi_scores": roi_scores,
                "roi_labels": roi_labels, "reg_valid_mask": reg_valid_mask, "rcnn_cls_labels": cls_labels}

    def sample_rois_for_rcnn(self, batch_dict):
        cfg = self.roi_sampler_cfg
        rois, roi_scores, roi_labels = batch_dict["rois"], batch_dict["roi_scores"], batch_dict["roi_labels"]
        gt = batch_dict["gt_boxes"]
        batch_size = int(batch_dict["batch_size"])
        if gt.shape[1] == 0:                 # no gt row at all: the reference's single zero row
            gt = gt.new_zeros((gt.shape[0], 1, gt.shape[2]))
        max_iou, gt_index = ops.roi_iou3d_max(rois, roi_labels, gt, cfg.get("SAMPLE_ROI_BY_EACH_CLASS", False))
        iou_host = max_iou.cpu()
        picks = torch.stack([self.subsample_rois(iou_host[b]) for b in range(batch_size)], 0)
        picks = picks.to(rois.device, non_blocking=True)

        def take(t, idx):
            if t.dim() == 2:
                return torch.gather(t, 1, idx)
            return torch.gather(t, 1, idx.unsqueeze(-1).expand(-1, -1, t.shape[-1]))

        gt_of_rois = take(gt, take(gt_index, picks))
        return take(rois, picks), gt_of_rois, take(max_iou, picks), take(roi_scores, picks), take(roi_labels, picks)

    def subsample_rois(self, max_overlaps):
        """max_overlaps: [N] CPU tensor -> ROI_PER_IMAGE indices (CPU int64): fg first, then hard and easy bg."""
        cfg = self.roi_sampler_cfg
        per_image = cfg.ROI_PER_IMAGE
        fg_per_image = int(np.round(cfg.FG_RATIO * per_image))
        fg_thresh = min(cfg.REG_FG_THRESH, cfg.CLS_FG_THRESH)

        fg_inds = (max_overlaps >= fg_thresh).nonzero().view(-1)
        easy_bg_inds = (max_overlaps < cfg.CLS_BG_THRESH_LO).nonzero().view(-1)
        hard_bg_inds = ((max_overlaps < cfg.REG_FG_THRESH) & (max_overlaps >= cfg.CLS_BG_THRESH_LO)).nonzero().view(-1)
        n_fg, n_bg = fg_inds.numel(), hard_bg_inds.numel() + easy_bg_inds.numel()

        if n_fg > 0 and n_bg > 0:
            n_fg_keep = min(fg_per_image, n_fg)
            order = torch.from_numpy(np.random.permutation(n_fg)).long()
            fg_inds = fg_inds[order[:n_fg_keep]]
            bg_inds = self.sample_bg_inds(hard_bg_inds, easy_bg_inds, per_image - n_fg_keep, cfg.HARD_BG_RATIO)
        elif n_fg > 0:
            draw = np.floor(np.random.rand(per_image) * n_fg)
            fg_inds = fg_inds[torch.from_numpy(draw).float().long()]
            bg_inds = fg_inds.new_zeros((0,))
        elif n_bg > 0:
            fg_inds = fg_inds.new_zeros((0,))
            bg_inds = self.sample_bg_inds(hard_bg_inds, easy_bg_inds, per_image, cfg.HARD_BG_RATIO)
        else:
            raise NotImplementedError(f"no fg and no bg roi among {max_overlaps.numel()}")
        return torch.cat((fg_inds, bg_inds), dim=0)

    @staticmethod
    def sample_bg_inds(hard_bg_inds, easy_bg_inds, n_bg, hard_bg_ratio):
        n_hard, n_easy = hard_bg_inds.numel(), easy_bg_inds.numel()
        if n_hard > 0 and n_easy > 0:
            take_hard = min(int(n_bg * hard_bg_ratio), n_hard)
            hard = hard_bg_inds[torch.randint(low=0, high=n_hard, size=(take_hard,)).long()]
            easy = easy_bg_inds[torch.randint(low=0, high=n_easy, size=(n_bg - take_hard,)).long()]
            return torch.cat([hard, easy], dim=0)
        if n_hard > 0:
            return hard_bg_inds[torch.randint(low=0, high=n_hard, size=(n_bg,)).long()]
        if n_easy > 0:
            return easy_bg_inds[torch.randint(low=0, high=n_easy, size=(n_bg,)).long()]
        raise NotImplementedError("no background roi to sample")
