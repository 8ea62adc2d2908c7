"""PVRCNN (reference pcdet/models/detectors/pv_rcnn.py:4-31): voxel backbone, dense-head RPN (AnchorHeadSingle or CenterHead),
VoxelSetAbstraction keypoints, PointHeadSimple and PVRCNNHead.  Training loss: RPN + point + rcnn.  The three modules are built
here, so the shared builders keep refusing PFE / POINT_HEAD sections and these heads for every other detector."""
from ..backbones_3d import pfe
from ..dense_heads.point_head_simple import PointHeadSimple
from ..roi_heads.pvrcnn_head import PVRCNNHead
from .detector3d_template import Detector3DTemplate


class PVRCNN(Detector3DTemplate):
    def __init__(self, model_cfg, num_class, dataset):
        super().__init__(model_cfg=model_cfg, num_class=num_class, dataset=dataset)
        self.module_list = self.build_networks()

    def build_pfe(self, model_info_dict):
        cfg = self._section("PFE")
        if cfg is None or cfg.NAME not in pfe.__all__:
            return super().build_pfe(model_info_dict)
        m = pfe.__all__[cfg.NAME](model_cfg=cfg, voxel_size=model_info_dict["voxel_size"], point_cloud_range=model_info_dict["point_cloud_range"],
                                  num_bev_features=model_info_dict["num_bev_features"],
                                  num_rawpoint_features=model_info_dict["num_rawpoint_features"])
        model_info_dict["module_list"].append(m)
        model_info_dict["num_point_features"] = m.num_point_features
        model_info_dict["num_point_features_before_fusion"] = m.num_point_features_before_fusion
        return m, model_info_dict

    def build_point_head(self, model_info_dict):
        cfg = self._section("POINT_HEAD")
        if cfg is None or cfg.NAME != "PointHeadSimple":
            return super().build_point_head(model_info_dict)
        key = "num_point_features_before_fusion" if cfg.get("USE_POINT_FEATURES_BEFORE_FUSION", False) else "num_point_features"
        m = PointHeadSimple(model_cfg=cfg, input_channels=model_info_dict[key], num_class=self.num_class if not cfg.CLASS_AGNOSTIC else 1,
                            predict_boxes_when_training=bool(self.model_cfg.get("ROI_HEAD", False)))
        model_info_dict["module_list"].append(m)
        return m, model_info_dict

    def build_roi_head(self, model_info_dict):
        """PVRCNNHead pools the keypoints: its input width is the PFE's num_point_features (reference detector3d_template.py:188-199)."""
        cfg = self._section("ROI_HEAD")
        if cfg is None or cfg.NAME != "PVRCNNHead":
            return super().build_roi_head(model_info_dict)
        m = PVRCNNHead(model_cfg=cfg, input_channels=model_info_dict["num_point_features"],
                       num_class=self.num_class if not cfg.CLASS_AGNOSTIC else 1)
        model_info_dict["module_list"].append(m)
        return m, model_info_dict

    def forward(self, batch_dict):
        for cur_module in self.module_list:
            batch_dict = cur_module(batch_dict)
        if self.training:
            loss, tb_dict, disp_dict = self.get_training_loss()
            return {"loss": loss}, tb_dict, disp_dict
        return self.post_processing(batch_dict)

    def get_training_loss(self):
        loss_rpn, tb_dict = self.dense_head.get_loss()
        tb_dict = {"loss_rpn": loss_rpn.detach(), **tb_dict}
        loss_point, tb_dict = self.point_head.get_loss(tb_dict)
        loss_rcnn, tb_dict = self.roi_head.get_loss(tb_dict)
        return loss_rpn + loss_point + loss_rcnn, tb_dict, {}
