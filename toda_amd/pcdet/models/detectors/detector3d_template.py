"""Detector3DTemplate (reference pcdet/models/detectors/detector3d_template.py:14-411): module
topology, registry-driven builders, checkpoint loading with the spconv-1.x -> 2.x weight layout
conversion.  The voxel / pillar topology is populated, with the registered RoI heads (roi_heads.__all__) on top; the pfe /
point_head builders refuse their sections (point-based detectors: out of scope)."""
import os

import torch
import torch.nn as nn

from ...utils.spconv_utils import find_all_spconv_keys
from .. import backbones_2d, backbones_3d, dense_heads, roi_heads
from ..backbones_2d import map_to_bev
from ..backbones_3d import vfe


class Detector3DTemplate(nn.Module):
    def __init__(self, model_cfg, num_class, dataset):
        super().__init__()
        self.model_cfg = model_cfg
        self.num_class = num_class
        self.dataset = dataset
        self.class_names = dataset.class_names
        self.register_buffer("global_step", torch.LongTensor(1).zero_())
        self.module_topology = ["vfe", "backbone_3d", "map_to_bev_module", "pfe", "backbone_2d", "dense_head",
                                "point_head", "roi_head"]

    @property
    def mode(self):
        return "TRAIN" if self.training else "TEST"

    def update_global_step(self):
        self.global_step += 1

    def __call__(self, *args, **kwargs):
        # the BatchNorm step counters of one forward are bumped by a single foreach launch (ops.bn_counter_scope)
        from .... import ops
        with ops.bn_counter_scope():
            return super().__call__(*args, **kwargs)

    def build_networks(self):
        enc = self.dataset.point_feature_encoder
        info = {
            "module_list": [],
            "num_rawpoint_features": enc.num_point_features,
            "num_point_features": enc.num_point_features,
            "grid_size": self.dataset.grid_size,
            "point_cloud_range": self.dataset.point_cloud_range,
            "voxel_size": self.dataset.voxel_size,
            "depth_downsample_factor": getattr(self.dataset, "depth_downsample_factor", None),
        }
        for name in self.module_topology:
            module, info = getattr(self, f"build_{name}")(model_info_dict=info)
            self.add_module(name, module)
        return info["module_list"]

    def _section(self, key):
        return self.model_cfg.get(key, None)

    def build_vfe(self, model_info_dict):
        cfg = self._section("VFE")
        if cfg is None:
            return None, model_info_dict
        m = vfe.__all__[cfg.NAME](
            model_cfg=cfg, num_point_features=model_info_dict["num_rawpoint_features"],
            point_cloud_range=model_info_dict["point_cloud_range"], voxel_size=model_info_dict["voxel_size"],
            grid_size=model_info_dict["grid_size"], depth_downsample_factor=model_info_dict["depth_downsample_factor"])
        model_info_dict["num_point_features"] = m.get_output_feature_dim()
        model_info_dict["module_list"].append(m)
        return m, model_info_dict

    def build_backbone_3d(self, model_info_dict):
        cfg = self._section("BACKBONE_3D")
        if cfg is None:
            return None, model_info_dict
        m = backbones_3d.__all__[cfg.NAME](
            model_cfg=cfg, input_channels=model_info_dict["num_point_features"],
            grid_size=model_info_dict["grid_size"], voxel_size=model_info_dict["voxel_size"],
            point_cloud_range=model_info_dict["point_cloud_range"])
        model_info_dict["module_list"].append(m)
        model_info_dict["num_point_features"] = m.num_point_features
        model_info_dict["backbone_channels"] = getattr(m, "backbone_channels", None)
        return m, model_info_dict

    def build_map_to_bev_module(self, model_info_dict):
        cfg = self._section("MAP_TO_BEV")
        if cfg is None:
            return None, model_info_dict
        m = map_to_bev.__all__[cfg.NAME](model_cfg=cfg, grid_size=model_info_dict["grid_size"])
        model_info_dict["module_list"].append(m)
        model_info_dict["num_bev_features"] = m.num_bev_features
        return m, model_info_dict

    def build_backbone_2d(self, model_info_dict):
        cfg = self._section("BACKBONE_2D")
        if cfg is None:
            return None, model_info_dict
        m = backbones_2d.__all__[cfg.NAME](model_cfg=cfg, input_channels=model_info_dict["num_bev_features"])
        model_info_dict["module_list"].append(m)
        model_info_dict["num_bev_features"] = m.num_bev_features
        return m, model_info_dict

    def build_dense_head(self, model_info_dict):
        cfg = self._section("DENSE_HEAD")
        if cfg is None:
            return None, model_info_dict
        m = dense_heads.__all__[cfg.NAME](
            model_cfg=cfg, input_channels=model_info_dict["num_bev_features"],
            num_class=self.num_class if not cfg.CLASS_AGNOSTIC else 1, class_names=self.class_names,
            grid_size=model_info_dict["grid_size"], point_cloud_range=model_info_dict["point_cloud_range"],
            predict_boxes_when_training=bool(self.model_cfg.get("ROI_HEAD", False)),
            voxel_size=model_info_dict.get("voxel_size", False))
        model_info_dict["module_list"].append(m)
        return m, model_info_dict

    def _unsupported(self, key, model_info_dict):
        if self._section(key) is not None:
            raise NotImplementedError(f"MODEL.{key} belongs to two-stage / point detectors: out of scope (DESIGN.md)")
        return None, model_info_dict

    def build_pfe(self, model_info_dict):
        return self._unsupported("PFE", model_info_dict)

    def build_point_head(self, model_info_dict):
        return self._unsupported("POINT_HEAD", model_info_dict)

    def build_roi_head(self, model_info_dict):
        cfg = self._section("ROI_HEAD")
        if cfg is None:
            return None, model_info_dict
        if cfg.NAME not in roi_heads.__all__:
            raise NotImplementedError(f"MODEL.ROI_HEAD {cfg.NAME}: only {sorted(roi_heads.__all__)} are on this path (DESIGN.md)")
        m = roi_heads.__all__[cfg.NAME](
            model_cfg=cfg, input_channels=model_info_dict["num_bev_features"],
            backbone_channels=model_info_dict.get("backbone_channels", None),
            point_cloud_range=model_info_dict["point_cloud_range"], voxel_size=model_info_dict["voxel_size"],
            num_class=self.num_class if not cfg.CLASS_AGNOSTIC else 1)
        model_info_dict["module_list"].append(m)
        return m, model_info_dict

    def forward(self, **kwargs):
        raise NotImplementedError

    # ------------------------------------------------------------- evaluation
    def post_processing(self, batch_dict):
        """Reference detector3d_template.py:178-284: per sample sigmoid scores, then either the best class and one
        class-agnostic rotated NMS, or (MULTI_CLASSES_NMS / the per-head score lists of a separate multi-head) one NMS per
        class with the heads' label mapping -> pred dicts, plus the recall record."""
        from ..model_utils import model_nms_utils

        cfg = self.model_cfg.POST_PROCESSING
        multi = cfg.NMS_CONFIG.get("MULTI_CLASSES_NMS", False)
        if isinstance(batch_dict["batch_cls_preds"], list) and not multi:
            raise NotImplementedError("per-head class scores (SEPARATE_MULTIHEAD) need NMS_CONFIG.MULTI_CLASSES_NMS: True")
        recall_dict, pred_dicts = {}, []
        for index in range(batch_dict["batch_size"]):
            if batch_dict.get("batch_index", None) is not None:
                pick = batch_dict["batch_index"] == index
            else:
                pick = index
            box_preds = batch_dict["batch_box_preds"][pick]
            if multi:
                heads = batch_dict["batch_cls_preds"]
                if isinstance(heads, list):
                    heads, mapping = [h[pick] for h in heads], batch_dict["multihead_label_mapping"]
                else:
                    heads, mapping = [heads[pick]], [torch.arange(1, self.num_class + 1, device=box_preds.device)]
                if not batch_dict["cls_preds_normalized"]:
                    heads = [torch.sigmoid(h) for h in heads]
                start, parts = 0, []
                for scores, labels_of in zip(heads, mapping):
                    assert scores.shape[1] == len(labels_of)
                    s, l, b = model_nms_utils.multi_classes_nms(cls_scores=scores, box_preds=box_preds[start:start + scores.shape[0]],
                                                                nms_config=cfg.NMS_CONFIG, score_thresh=cfg.SCORE_THRESH)
                    parts.append((s, labels_of.to(l.device)[l], b))
                    start += scores.shape[0]
                final_scores, final_labels, final_boxes = (torch.cat([p[i] for p in parts], dim=0) for i in range(3))
                recall_dict = self.generate_recall_record(final_boxes if "rois" not in batch_dict else box_preds, recall_dict, index,
                                                          batch_dict, cfg.RECALL_THRESH_LIST)
                pred_dicts.append({"pred_boxes": final_boxes, "pred_scores": final_scores, "pred_labels": final_labels})
                continue
            raw_cls = batch_dict["batch_cls_preds"][pick]
            cls_preds = raw_cls if batch_dict["cls_preds_normalized"] else torch.sigmoid(raw_cls)
            scores, labels = torch.max(cls_preds, dim=-1)
            if batch_dict.get("has_class_labels", False):
                # two-stage detectors: the labels of the rois the scores refine (reference :252-256)
                labels = batch_dict["roi_labels" if "roi_labels" in batch_dict else "batch_pred_labels"][index]
            else:
                labels = labels + 1
            selected, selected_scores = model_nms_utils.class_agnostic_nms(box_scores=scores, box_preds=box_preds,
                                                                           nms_config=cfg.NMS_CONFIG, score_thresh=cfg.SCORE_THRESH)
            if cfg.get("OUTPUT_RAW_SCORE", False):
                selected_scores = torch.max(raw_cls, dim=-1)[0][selected]
            final_boxes = box_preds[selected]
            recall_dict = self.generate_recall_record(final_boxes if "rois" not in batch_dict else box_preds, recall_dict, index, batch_dict,
                                                      cfg.RECALL_THRESH_LIST)
            pred_dicts.append({"pred_boxes": final_boxes, "pred_scores": selected_scores, "pred_labels": labels[selected]})
        return pred_dicts, recall_dict

    @staticmethod
    def generate_recall_record(box_preds, recall_dict, batch_index, data_dict=None, thresh_list=None):
        """#gt boxes whose best 3-D IoU with a prediction (rcnn_*) or, for two-stage detectors, with a roi (roi_*) exceeds each
        threshold (reference :286-328); trailing all-zero rows of the padded gt tensor are ignored, as there."""
        from ...ops.iou3d_nms import iou3d_nms_utils

        if "gt_boxes" not in data_dict:
            return recall_dict
        if len(recall_dict) == 0:
            recall_dict = {"gt": 0}
            for t in thresh_list:
                recall_dict[f"roi_{t}"] = 0
                recall_dict[f"rcnn_{t}"] = 0
        gt = data_dict["gt_boxes"][batch_index]
        k = gt.shape[0] - 1
        while k > 0 and float(gt[k].sum()) == 0:
            k -= 1
        gt = gt[:k + 1]
        if gt.shape[0] > 0:
            if box_preds.shape[0] > 0:
                best = iou3d_nms_utils.boxes_iou3d_gpu(box_preds[:, 0:7].contiguous(), gt[:, 0:7].contiguous()).max(dim=0)[0]
                for t in thresh_list:
                    recall_dict[f"rcnn_{t}"] += int((best > t).sum().item())
            if "rois" in data_dict:
                rois = data_dict["rois"][batch_index]
                best = iou3d_nms_utils.boxes_iou3d_gpu(rois[:, 0:7].contiguous(), gt[:, 0:7].contiguous()).max(dim=0)[0]
                for t in thresh_list:
                    recall_dict[f"roi_{t}"] += int((best > t).sum().item())
            recall_dict["gt"] += gt.shape[0]
        return recall_dict

    # ------------------------------------------------------------- checkpoints
    def _load_state_dict(self, model_state_disk, *, strict=True):
        """Accept spconv-1.x weights [kz,ky,kx,Cin,Cout] into our spconv-2.x [Cout,kz,ky,kx,Cin]
        parameters (reference :330-359); keys whose shape still differs are skipped."""
        state = self.state_dict()
        spconv_keys = find_all_spconv_keys(self)
        update = {}
        for key, val in model_state_disk.items():
            if key in spconv_keys and key in state and state[key].shape != val.shape:
                if val.dim() == 5:
                    native = val.transpose(-1, -2)           # [k,k,k,Cout,Cin]
                    if native.shape == state[key].shape:
                        val = native.contiguous()
                    else:
                        implicit = val.permute(4, 0, 1, 2, 3)  # [Cout,k,k,k,Cin]
                        if implicit.shape == state[key].shape:
                            val = implicit.contiguous()
            if key in state and state[key].shape == val.shape:
                update[key] = val
        if strict:
            self.load_state_dict(update)
        else:
            state.update(update)
            self.load_state_dict(state)
        return state, update

    def load_params_from_file(self, filename, logger=None, to_cpu=False):
        if not os.path.isfile(filename):
            raise FileNotFoundError(filename)
        ckpt = torch.load(filename, map_location=torch.device("cpu") if to_cpu else None)
        state, update = self._load_state_dict(ckpt["model_state"], strict=False)
        if logger is not None:
            for key in state:
                if key not in update:
                    logger.info(f"Not updated weight {key}: {tuple(state[key].shape)}")
            logger.info(f"==> Done (loaded {len(update)}/{len(state)})")

    def load_params_with_optimizer(self, filename, to_cpu=False, optimizer=None, logger=None):
        if not os.path.isfile(filename):
            raise FileNotFoundError(filename)
        ckpt = torch.load(filename, map_location=torch.device("cpu") if to_cpu else None)
        self._load_state_dict(ckpt["model_state"], strict=True)
        if optimizer is not None and ckpt.get("optimizer_state") is not None:
            optimizer.load_state_dict(ckpt["optimizer_state"])
        return ckpt.get("it", 0.0), ckpt.get("epoch", -1)
