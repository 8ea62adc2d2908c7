"""SECONDNetIoU (reference pcdet/models/detectors/second_net_iou.py:7-177): SECOND + AnchorHeadSingle proposals rescored by
SECONDHead's IoU prediction."""
import torch

from toda_amd import ops

from ..model_utils.model_nms_utils import class_agnostic_nms
from .detector3d_template import Detector3DTemplate


class SECONDNetIoU(Detector3DTemplate):
    def __init__(self, model_cfg, num_class, dataset):
        super().__init__(model_cfg=model_cfg, num_class=num_class, dataset=dataset)
        self.module_list = self.build_networks()

    def forward(self, batch_dict):
        batch_dict["dataset_cfg"] = self.dataset.dataset_cfg
        for module in self.module_list:
            batch_dict = module(batch_dict)
        if self.training:
            loss, tb_dict, disp_dict = self.get_training_loss()
            if getattr(self, "return_batch_dict", False):
                # the stage-2 consistency step filters the dense predictions itself (models.filter_boxes_secondiou)
                return batch_dict, {"loss": loss}, tb_dict, disp_dict
            return {"loss": loss}, tb_dict, disp_dict
        return self.post_processing(batch_dict)

    def get_training_loss(self):
        loss_rpn, tb_dict = self.dense_head.get_loss()
        tb_dict = {"loss_rpn": loss_rpn.detach(), **tb_dict}
        loss_rcnn, tb_dict = self.roi_head.get_loss(tb_dict)
        return loss_rpn + loss_rcnn, tb_dict, {}

    @staticmethod
    def cal_scores_by_npoints(cls_scores, iou_scores, num_points_in_gt, cls_thresh=10, iou_thresh=100):
        """Blend of the classification and IoU scores by the number of points in the box (reference :29-48, including its
        fixed offset of 10 points in the ramp)."""
        assert iou_thresh >= cls_thresh
        alpha = torch.zeros(cls_scores.shape, dtype=torch.float32, device=cls_scores.device)
        alpha = torch.where(num_points_in_gt >= iou_thresh, torch.ones_like(alpha), alpha)
        ramp = (num_points_in_gt > cls_thresh) & (num_points_in_gt < iou_thresh)
        alpha = torch.where(ramp, (num_points_in_gt - 10) / (iou_thresh - cls_thresh), alpha)
        return (1 - alpha) * cls_scores + alpha * iou_scores

    def set_nms_score_by_class(self, iou_preds, cls_preds, label_preds, score_by_class):
        n_classes = torch.unique(label_preds).shape[0]
        nms_scores = torch.zeros(iou_preds.shape, dtype=torch.float32, device=iou_preds.device)
        for i in range(n_classes):
            mask = label_preds == (i + 1)
            score_type = score_by_class[self.class_names[i]]
            if score_type == "iou":
                nms_scores = torch.where(mask, iou_preds, nms_scores)
            elif score_type == "cls":
                nms_scores = torch.where(mask, cls_preds, nms_scores)
            else:
                raise NotImplementedError(score_type)
        return nms_scores

    @staticmethod
    def points_per_box(points, boxes):
        """points [P, 3], boxes [K, 7] (device) -> [K] float: points inside each box (roiaware test, as points_in_boxes_cpu)."""
        if boxes.shape[0] == 0:
            return boxes.new_zeros((0,))
        pts = points.contiguous().float()
        return torch.stack([ops.points_in_boxes(pts, boxes[k:k + 1].contiguous(), mode=0).sum() for k in range(boxes.shape[0])]).float()

    def post_processing(self, batch_dict):
        """Per sample: sigmoid of the IoU and roi scores, the configured NMS score, class-agnostic rotated NMS, pred dicts with
        pred_boxes / pred_scores / pred_labels / pred_cls_scores / pred_iou_scores, and the recall record (rois and final boxes)."""
        cfg = self.model_cfg.POST_PROCESSING
        nms_cfg = cfg.NMS_CONFIG
        recall_dict, pred_dicts = {}, []
        for index in range(batch_dict["batch_size"]):
            if batch_dict.get("batch_index", None) is not None:
                assert batch_dict["batch_cls_preds"].dim() == 2
                pick = batch_dict["batch_index"] == index
            else:
                assert batch_dict["batch_cls_preds"].dim() == 3
                pick = index
            box_preds = batch_dict["batch_box_preds"][pick]
            iou_preds = batch_dict["batch_cls_preds"][pick]
            cls_preds = batch_dict["roi_scores"][pick]
            src_box_preds = box_preds
            assert iou_preds.shape[1] in [1, self.num_class]
            if not batch_dict["cls_preds_normalized"]:
                iou_preds, cls_preds = torch.sigmoid(iou_preds), torch.sigmoid(cls_preds)
            if nms_cfg.MULTI_CLASSES_NMS:
                raise NotImplementedError("multi-class NMS is not on this path")
            iou_preds, label_preds = torch.max(iou_preds, dim=-1)
            label_preds = batch_dict["roi_labels"][index] if batch_dict.get("has_class_labels", False) else label_preds + 1

            score_type = nms_cfg.get("SCORE_TYPE", None)
            if nms_cfg.get("SCORE_BY_CLASS", None) and score_type == "score_by_class":
                nms_scores = self.set_nms_score_by_class(iou_preds, cls_preds, label_preds, nms_cfg.SCORE_BY_CLASS)
            elif score_type in ("iou", None):
                nms_scores = iou_preds
            elif score_type == "cls":
                nms_scores = cls_preds
            elif score_type == "weighted_iou_cls":
                nms_scores = nms_cfg.SCORE_WEIGHTS.iou * iou_preds + nms_cfg.SCORE_WEIGHTS.cls * cls_preds
            elif score_type == "num_pts_iou_cls":
                points = batch_dict["points"]
                sample_points = points[points[:, 0] == index][:, 1:4]
                n_pts = self.points_per_box(sample_points, box_preds[:, 0:7])
                nms_scores = self.cal_scores_by_npoints(cls_preds, iou_preds, n_pts, nms_cfg.SCORE_THRESH.cls, nms_cfg.SCORE_THRESH.iou)
            else:
                raise NotImplementedError(f"SCORE_TYPE {score_type}")

            selected, selected_scores = class_agnostic_nms(box_scores=nms_scores, box_preds=box_preds, nms_config=nms_cfg,
                                                           score_thresh=cfg.SCORE_THRESH)
            if cfg.OUTPUT_RAW_SCORE:
                raise NotImplementedError("OUTPUT_RAW_SCORE")
            final_boxes = box_preds[selected]
            recall_dict = self.generate_recall_record(final_boxes if "rois" not in batch_dict else src_box_preds, recall_dict, index,
                                                      batch_dict, cfg.RECALL_THRESH_LIST)
            pred_dicts.append({"pred_boxes": final_boxes, "pred_scores": selected_scores, "pred_labels": label_preds[selected],
                               "pred_cls_scores": cls_preds[selected], "pred_iou_scores": iou_preds[selected]})
        return pred_dicts, recall_dict
