"""VoxelRCNNHead (reference pcdet/models/roi_heads/voxelrcnn_head.py:8-261): the voxel RoI grid pool of Voxel R-CNN.

Each roi carries a G x G x G grid of points; per feature level (x_conv2..4 of VoxelBackBone8x) a NeighborVoxelSAModuleMSG
pools the level's voxels around every grid point (voxel query + fused neighbour pool in HIP on CUDA tensors, the plain-torch
restatement on CPU tensors).  The pooled layout stays the reference's [R, G^3, sum C], so the first shared_fc_layer weight lines up
with reference checkpoints.  Unlike SECONDHead's pool this one is trained end to end: gradients flow back into the levels."""
import torch
import torch.nn as nn

from ...ops.pointnet2.pointnet2_stack import voxel_pool_modules as voxelpool_stack_modules
from ...ops.pointnet2.pointnet2_stack.voxel_query_utils import VoxelLevel
from ...utils import common_utils
from .roi_head_template import RoIHeadTemplate
from .second_head import run_fc_rows


class VoxelRCNNHead(RoIHeadTemplate):
    def __init__(self, backbone_channels, model_cfg, point_cloud_range, voxel_size, num_class=1, **kwargs):
        super().__init__(num_class=num_class, model_cfg=model_cfg)
        self.model_cfg = model_cfg
        self.pool_cfg = model_cfg.ROI_GRID_POOL
        layer_cfg = self.pool_cfg.POOL_LAYERS
        self.point_cloud_range = point_cloud_range
        self.voxel_size = voxel_size

        c_out = 0
        self.roi_grid_pool_layers = nn.ModuleList()
        for src_name in self.pool_cfg.FEATURES_SOURCE:
            mlps = [[backbone_channels[src_name]] + list(m) for m in layer_cfg[src_name].MLPS]
            self.roi_grid_pool_layers.append(voxelpool_stack_modules.NeighborVoxelSAModuleMSG(
                query_ranges=layer_cfg[src_name].QUERY_RANGES, nsamples=layer_cfg[src_name].NSAMPLE,
                radii=layer_cfg[src_name].POOL_RADIUS, mlps=mlps, pool_method=layer_cfg[src_name].POOL_METHOD))
            c_out += sum(m[-1] for m in mlps)

        g = self.pool_cfg.GRID_SIZE
        pre_channel = g * g * g * c_out
        self.shared_fc_layer, pre_channel = self._fc_stack(pre_channel, model_cfg.SHARED_FC, inplace=True)
        self.cls_fc_layers, pre_cls = self._fc_stack(pre_channel, model_cfg.CLS_FC)
        self.cls_pred_layer = nn.Linear(pre_cls, self.num_class, bias=True)
        self.reg_fc_layers, pre_reg = self._fc_stack(pre_channel, model_cfg.REG_FC)
        self.reg_pred_layer = nn.Linear(pre_reg, self.box_coder.code_size * self.num_class, bias=True)
        self.init_weights()

    def _fc_stack(self, pre_channel, widths, inplace=False):
        """[Linear (no bias), BatchNorm1d, ReLU] per width, Dropout(DP_RATIO) between them when DP_RATIO > 0."""
        layers = []
        for k, width in enumerate(widths):
            layers += [nn.Linear(pre_channel, width, bias=False), nn.BatchNorm1d(width), nn.ReLU(inplace=inplace)]
            pre_channel = width
            if k != len(widths) - 1 and self.model_cfg.DP_RATIO > 0:
                layers.append(nn.Dropout(self.model_cfg.DP_RATIO))
        return nn.Sequential(*layers), pre_channel

    def init_weights(self):
        for module_list in [self.shared_fc_layer, self.cls_fc_layers, self.reg_fc_layers]:
            for m in module_list.modules():
                if isinstance(m, nn.Linear):
                    nn.init.xavier_normal_(m.weight)
                    if m.bias is not None:
                        nn.init.constant_(m.bias, 0)
        nn.init.normal_(self.cls_pred_layer.weight, 0, 0.01)
        nn.init.constant_(self.cls_pred_layer.bias, 0)
        nn.init.normal_(self.reg_pred_layer.weight, mean=0, std=0.001)
        nn.init.constant_(self.reg_pred_layer.bias, 0)

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
        """rois [B, N, 7 + C] + multi_scale_3d_features -> [B * N, G^3, sum C] (reference voxelrcnn_head.py:106-197)."""
        rois = batch_dict["rois"]
        batch_size = batch_dict["batch_size"]
        if batch_dict.get("with_voxel_feature_transform", False):
            raise NotImplementedError("VoxelRCNNHead: with_voxel_feature_transform (multi_scale_3d_features_post) is not on this path")
        roi_grid_xyz, _ = self.get_global_grid_points_of_roi(rois, grid_size=self.pool_cfg.GRID_SIZE)
        roi_grid_xyz = roi_grid_xyz.view(batch_size, -1, 3)
        # voxel coordinates of the grid points: torch's floor division of floats, as the reference
        roi_grid_coords_x = (roi_grid_xyz[:, :, 0:1] - self.point_cloud_range[0]) // self.voxel_size[0]
        roi_grid_coords_y = (roi_grid_xyz[:, :, 1:2] - self.point_cloud_range[1]) // self.voxel_size[1]
        roi_grid_coords_z = (roi_grid_xyz[:, :, 2:3] - self.point_cloud_range[2]) // self.voxel_size[2]
        roi_grid_coords = torch.cat([roi_grid_coords_x, roi_grid_coords_y, roi_grid_coords_z], dim=-1)
        batch_idx = rois.new_zeros(batch_size, roi_grid_coords.shape[1], 1)
        for bs_idx in range(batch_size):
            batch_idx[bs_idx, :, 0] = bs_idx
        new_xyz = roi_grid_xyz.contiguous().view(-1, 3)

        pooled_features_list = []
        for k, src_name in enumerate(self.pool_cfg.FEATURES_SOURCE):
            pool_layer = self.roi_grid_pool_layers[k]
            cur_stride = batch_dict["multi_scale_3d_strides"][src_name]
            cur_sp_tensors = batch_dict["multi_scale_3d_features"][src_name]
            cur_coords = cur_sp_tensors.indices
            cur_voxel_xyz = common_utils.get_voxel_centers(cur_coords[:, 1:4], downsample_times=cur_stride, voxel_size=self.voxel_size,
                                                           point_cloud_range=self.point_cloud_range)
            level = VoxelLevel(cur_coords, cur_sp_tensors.spatial_shape, batch_size, getattr(cur_sp_tensors, "grid_index", None))
            cur_roi_grid_coords = torch.cat([batch_idx, roi_grid_coords // cur_stride], dim=-1).int()
            # no per-sample counts: the query returns rows of the level's table, batch offsets included (the reference's
            # xyz_batch_cnt / new_xyz_batch_cnt only serve its stack grouping, and counting the rows would cost a host sync)
            pooled = pool_layer(xyz=cur_voxel_xyz.contiguous(), xyz_batch_cnt=None, new_xyz=new_xyz, new_xyz_batch_cnt=None,
                                new_coords=cur_roi_grid_coords.contiguous().view(-1, 4),
                                features=cur_sp_tensors.features.contiguous(), level=level)
            if getattr(cur_sp_tensors, "grid_index", None) is None and level.grid_index is not None:
                cur_sp_tensors.grid_index = level.grid_index        # a level pooled twice (eval after train) builds its index once
            pooled_features_list.append(pooled.view(-1, self.pool_cfg.GRID_SIZE ** 3, pooled.shape[-1]))
        return torch.cat(pooled_features_list, dim=-1)

    def forward(self, batch_dict):
        targets_dict = self.proposal_layer(batch_dict, nms_config=self.model_cfg.NMS_CONFIG["TRAIN" if self.training else "TEST"])
        if self.training:
            targets_dict = self.assign_targets(batch_dict)
            batch_dict["rois"] = targets_dict["rois"]
            batch_dict["roi_labels"] = targets_dict["roi_labels"]

        pooled_features = self.roi_grid_pool(batch_dict)                        # (R, G^3, C)
        pooled_features = pooled_features.view(pooled_features.size(0), -1)
        shared_features = run_fc_rows(self.shared_fc_layer, pooled_features)
        rcnn_cls = self.cls_pred_layer(run_fc_rows(self.cls_fc_layers, shared_features))
        rcnn_reg = self.reg_pred_layer(run_fc_rows(self.reg_fc_layers, shared_features))

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
