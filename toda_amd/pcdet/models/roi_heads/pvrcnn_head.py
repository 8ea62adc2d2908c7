"""PVRCNNHead (reference pcdet/models/roi_heads/pvrcnn_head.py:7-175): the RoI-grid pool of PV-RCNN.  Every roi carries a
G x G x G grid of points; a StackSAModuleMSG pools the keypoints (VoxelSetAbstraction's point_features weighted by PointHeadSimple's
point_cls_scores) around each grid point.  The fc layers keep the reference's Conv1d / BatchNorm1d modules and state-dict keys and
run as matmuls on the [R, C] view, as SECONDHead and VoxelRCNNHead do."""
import torch
import torch.nn as nn

from ...ops.pointnet2.pointnet2_stack import pointnet2_modules as pointnet2_stack_modules
from ...utils import common_utils
from .roi_head_template import RoIHeadTemplate
from .second_head import run_fc_rows


class PVRCNNHead(RoIHeadTemplate):
    def __init__(self, input_channels, model_cfg, num_class=1, **kwargs):
        super().__init__(num_class=num_class, model_cfg=model_cfg)
        self.model_cfg = model_cfg
        self.roi_grid_pool_layer, num_c_out = pointnet2_stack_modules.build_local_aggregation_module(
            input_channels=input_channels, config=model_cfg.ROI_GRID_POOL)
        g = model_cfg.ROI_GRID_POOL.GRID_SIZE
        pre_channel = g * g * g * num_c_out
        shared_fc_list = []
        for k in range(len(model_cfg.SHARED_FC)):
            shared_fc_list.extend([nn.Conv1d(pre_channel, model_cfg.SHARED_FC[k], kernel_size=1, bias=False),
                                   nn.BatchNorm1d(model_cfg.SHARED_FC[k]), nn.ReLU()])
            pre_channel = model_cfg.SHARED_FC[k]
            if k != len(model_cfg.SHARED_FC) - 1 and model_cfg.DP_RATIO > 0:
                shared_fc_list.append(nn.Dropout(model_cfg.DP_RATIO))
        self.shared_fc_layer = nn.Sequential(*shared_fc_list)
        self.cls_layers = self.make_fc_layers(input_channels=pre_channel, output_channels=self.num_class, fc_list=model_cfg.CLS_FC)
        self.reg_layers = self.make_fc_layers(input_channels=pre_channel, output_channels=self.box_coder.code_size * self.num_class,
                                              fc_list=model_cfg.REG_FC)
        self.init_weights(weight_init="xavier")

    def init_weights(self, weight_init="xavier"):
        init_func = {"kaiming": nn.init.kaiming_normal_, "xavier": nn.init.xavier_normal_, "normal": nn.init.normal_}[weight_init]
        for m in self.modules():
            if isinstance(m, (nn.Conv2d, nn.Conv1d)):
                if weight_init == "normal":
                    init_func(m.weight, mean=0, std=0.001)
                else:
                    init_func(m.weight)
                if m.bias is not None:
                    nn.init.constant_(m.bias, 0)
        nn.init.normal_(self.reg_layers[-1].weight, mean=0, std=0.001)

    @staticmethod
    def get_dense_grid_points(rois, batch_size_rcnn, grid_size):
        faked_features = rois.new_ones((grid_size, grid_size, grid_size))
        dense_idx = faked_features.nonzero().repeat(batch_size_rcnn, 1, 1).float()      # (R, G^3, 3) [x_idx, y_idx, z_idx]
        local_roi_size = rois.view(batch_size_rcnn, -1)[:, 3:6]
        return (dense_idx + 0.5) / grid_size * local_roi_size.unsqueeze(dim=1) - (local_roi_size.unsqueeze(dim=1) / 2)

    def get_global_grid_points_of_roi(self, rois, grid_size):
        rois = rois.view(-1, rois.shape[-1])
        batch_size_rcnn = rois.shape[0]
        local_roi_grid_points = self.get_dense_grid_points(rois, batch_size_rcnn, grid_size)
        global_roi_grid_points = common_utils.rotate_points_along_z(local_roi_grid_points.clone(), rois[:, 6]).squeeze(dim=1)
        global_roi_grid_points += rois[:, 0:3].clone().unsqueeze(dim=1)
        return global_roi_grid_points, local_roi_grid_points

    def roi_grid_pool(self, batch_dict):
        """rois [B, N, 7 + C], keypoints (point_coords, point_features, point_cls_scores) -> [B N, G^3, C] (reference :77-123)."""
        batch_size = batch_dict["batch_size"]
        rois = batch_dict["rois"]
        point_coords = batch_dict["point_coords"]
        point_features = batch_dict["point_features"] * batch_dict["point_cls_scores"].view(-1, 1)
        global_roi_grid_points, _ = self.get_global_grid_points_of_roi(rois, grid_size=self.model_cfg.ROI_GRID_POOL.GRID_SIZE)
        global_roi_grid_points = global_roi_grid_points.view(batch_size, -1, 3)
        xyz = point_coords[:, 1:4]
        bidx = point_coords[:, 0].long()
        xyz_batch_cnt = torch.bincount(bidx, minlength=batch_size)[:batch_size].tolist()
        assert bidx.numel() < 2 or not bool((bidx[1:] < bidx[:-1]).any()), "PVRCNNHead: keypoints must be stacked sample after sample"
        new_xyz = global_roi_grid_points.view(-1, 3)
        new_xyz_batch_cnt = [global_roi_grid_points.shape[1]] * batch_size
        _, pooled_features = self.roi_grid_pool_layer(xyz=xyz.contiguous(), xyz_batch_cnt=xyz_batch_cnt, new_xyz=new_xyz.contiguous(),
                                                      new_xyz_batch_cnt=new_xyz_batch_cnt, features=point_features.contiguous())
        return pooled_features.view(-1, self.model_cfg.ROI_GRID_POOL.GRID_SIZE ** 3, pooled_features.shape[-1])

    def forward(self, batch_dict):
        targets_dict = self.proposal_layer(batch_dict, nms_config=self.model_cfg.NMS_CONFIG["TRAIN" if self.training else "TEST"])
        if self.training:
            targets_dict = batch_dict.get("roi_targets_dict", None)
            if targets_dict is None:
                targets_dict = self.assign_targets(batch_dict)
                batch_dict["rois"] = targets_dict["rois"]
                batch_dict["roi_labels"] = targets_dict["roi_labels"]

        pooled_features = self.roi_grid_pool(batch_dict)                        # (R, G^3, C)
        r = pooled_features.shape[0]
        # the reference's (R, C, G, G, G) flattening order, so the first shared_fc weight lines up with its checkpoints
        pooled_features = pooled_features.permute(0, 2, 1).contiguous().view(r, -1)
        shared_features = run_fc_rows(self.shared_fc_layer, pooled_features)
        rcnn_cls = run_fc_rows(self.cls_layers, shared_features)
        rcnn_reg = run_fc_rows(self.reg_layers, shared_features)

        if not self.training:
            batch_cls_preds, batch_box_preds = self.generate_predicted_boxes(batch_size=batch_dict["batch_size"], rois=batch_dict["rois"],
                                                                             cls_preds=rcnn_cls, box_preds=rcnn_reg)
            batch_dict["batch_cls_preds"] = batch_cls_preds
            batch_dict["batch_box_preds"] = batch_box_preds
            batch_dict["cls_preds_normalized"] = False
        else:
            targets_dict["rcnn_cls"] = rcnn_cls
            targets_dict["rcnn_reg"] = rcnn_reg
            self.forward_ret_dict = targets_dict
        return batch_dict
