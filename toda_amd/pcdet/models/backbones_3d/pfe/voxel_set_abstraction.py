"""VoxelSetAbstraction (reference pcdet/models/backbones_3d/pfe/voxel_set_abstraction.py:117-411): FPS keypoints per sample,
their features from the BEV map (bilinear interpolation), the sparse levels x_conv1..4 and the raw points (StackSAModuleMSG),
fused by Linear + BatchNorm1d + ReLU.  Module names and state-dict keys are the reference's.  CUDA tensors run the HIP kernels
(ops.farthest_point_sample, ops.bev_interpolate, the SA pool); CPU tensors their plain-torch restatements."""
import torch
import torch.nn as nn

from ....ops.pointnet2.pointnet2_stack import pointnet2_modules as pointnet2_stack_modules
from ....ops.pointnet2.pointnet2_stack import pointnet2_utils as pointnet2_stack_utils
from ....utils import common_utils
from toda_amd import ops


def bilinear_interpolate_torch(im, x, y):
    """im [H, W, C], x / y [N] -> [N, C] (reference :11-42)."""
    x0 = torch.floor(x).long()
    x1 = x0 + 1
    y0 = torch.floor(y).long()
    y1 = y0 + 1
    x0 = torch.clamp(x0, 0, im.shape[1] - 1)
    x1 = torch.clamp(x1, 0, im.shape[1] - 1)
    y0 = torch.clamp(y0, 0, im.shape[0] - 1)
    y1 = torch.clamp(y1, 0, im.shape[0] - 1)
    Ia = im[y0, x0]
    Ib = im[y1, x0]
    Ic = im[y0, x1]
    Id = im[y1, x1]
    wa = (x1.type_as(x) - x) * (y1.type_as(y) - y)
    wb = (x1.type_as(x) - x) * (y - y0.type_as(y))
    wc = (x - x0.type_as(x)) * (y1.type_as(y) - y)
    wd = (x - x0.type_as(x)) * (y - y0.type_as(y))
    return torch.t((torch.t(Ia) * wa)) + torch.t(torch.t(Ib) * wb) + torch.t(torch.t(Ic) * wc) + torch.t(torch.t(Id) * wd)


def _counts(batch_idx, batch_size):
    """(per-sample row counts, whether the stack is batch-contiguous) in one host read."""
    b = batch_idx.long()
    unsorted = (b[1:] < b[:-1]).any().view(1).long() if b.numel() > 1 else b.new_zeros(1)
    vals = torch.cat([torch.bincount(b, minlength=batch_size)[:batch_size], unsorted]).tolist()
    return vals[:batch_size], not vals[batch_size]


class VoxelSetAbstraction(nn.Module):
    def __init__(self, model_cfg, voxel_size, point_cloud_range, num_bev_features=None, num_rawpoint_features=None, **kwargs):
        super().__init__()
        self.model_cfg = model_cfg
        self.voxel_size = voxel_size
        self.point_cloud_range = point_cloud_range
        if model_cfg.get("SAMPLE_METHOD", "FPS") != "FPS":
            raise NotImplementedError(f"VoxelSetAbstraction SAMPLE_METHOD {model_cfg.SAMPLE_METHOD}: only FPS (SPC belongs to PV-RCNN++)")
        if model_cfg.POINT_SOURCE not in ("raw_points", "voxel_centers"):
            raise NotImplementedError(f"VoxelSetAbstraction POINT_SOURCE {model_cfg.POINT_SOURCE}")
        SA_cfg = model_cfg.SA_LAYER
        for src_name in model_cfg.FEATURES_SOURCE:
            if src_name != "bev" and SA_cfg[src_name].get("FILTER_NEIGHBOR_WITH_ROI", False):
                raise NotImplementedError("VoxelSetAbstraction FILTER_NEIGHBOR_WITH_ROI is out of scope")

        self.SA_layers = nn.ModuleList()
        self.SA_layer_names = []
        self.downsample_times_map = {}
        c_in = 0
        for src_name in model_cfg.FEATURES_SOURCE:
            if src_name in ["bev", "raw_points"]:
                continue
            self.downsample_times_map[src_name] = SA_cfg[src_name].DOWNSAMPLE_FACTOR
            if SA_cfg[src_name].get("INPUT_CHANNELS", None) is None:
                mlps0 = SA_cfg[src_name].MLPS[0]
                input_channels = mlps0[0] if isinstance(mlps0, list) else mlps0
            else:
                input_channels = SA_cfg[src_name]["INPUT_CHANNELS"]
            layer, c_out = pointnet2_stack_modules.build_local_aggregation_module(input_channels=input_channels, config=SA_cfg[src_name])
            self.SA_layers.append(layer)
            self.SA_layer_names.append(src_name)
            c_in += c_out
        if "bev" in model_cfg.FEATURES_SOURCE:
            c_in += num_bev_features
        if "raw_points" in model_cfg.FEATURES_SOURCE:
            self.SA_rawpoints, c_out = pointnet2_stack_modules.build_local_aggregation_module(
                input_channels=num_rawpoint_features - 3, config=SA_cfg["raw_points"])
            c_in += c_out
        self.vsa_point_feature_fusion = nn.Sequential(
            nn.Linear(c_in, model_cfg.NUM_OUTPUT_FEATURES, bias=False),
            nn.BatchNorm1d(model_cfg.NUM_OUTPUT_FEATURES),
            nn.ReLU(),
        )
        self.num_point_features = model_cfg.NUM_OUTPUT_FEATURES
        self.num_point_features_before_fusion = c_in

    def interpolate_from_bev_features(self, keypoints, bev_features, batch_size, bev_stride):
        x_idxs = (keypoints[:, 1] - self.point_cloud_range[0]) / self.voxel_size[0]
        y_idxs = (keypoints[:, 2] - self.point_cloud_range[1]) / self.voxel_size[1]
        x_idxs = x_idxs / bev_stride
        y_idxs = y_idxs / bev_stride
        if bev_features.is_cuda:
            return ops.bev_interpolate(bev_features, x_idxs, y_idxs, keypoints[:, 0])
        out = []
        for k in range(batch_size):
            bs_mask = keypoints[:, 0] == k
            out.append(bilinear_interpolate_torch(bev_features[k].permute(1, 2, 0), x_idxs[bs_mask], y_idxs[bs_mask]))
        return torch.cat(out, dim=0)

    def get_sampled_points(self, batch_dict):
        """keypoints [B x NUM_KEYPOINTS, 4] (bs_idx, x, y, z); one FPS launch for the whole batch on CUDA tensors."""
        batch_size = batch_dict["batch_size"]
        if self.model_cfg.POINT_SOURCE == "raw_points":
            src_points = batch_dict["points"][:, 1:4]
            batch_indices = batch_dict["points"][:, 0].long()
        else:
            src_points = common_utils.get_voxel_centers(batch_dict["voxel_coords"][:, 1:4], downsample_times=1, voxel_size=self.voxel_size,
                                                        point_cloud_range=self.point_cloud_range)
            batch_indices = batch_dict["voxel_coords"][:, 0].long()
        nk = self.model_cfg.NUM_KEYPOINTS
        counts, contiguous = _counts(batch_indices, batch_size)
        src = src_points.contiguous()
        if not contiguous:
            src = src[torch.argsort(batch_indices, stable=True)]
        idx = pointnet2_stack_utils.stack_farthest_point_sample_counts(src, counts, nk).long()
        keypoints, start = [], 0
        for k in range(batch_size):
            cur = idx[k]
            n = counts[k]
            if n < nk:       # reference :257-260: repeat the first N indices
                times = int(nk / max(n, 1)) + 1
                cur = cur[:n].repeat(times)[:nk]
            keypoints.append(src[start:start + n][cur])
            start += n
        keypoints = torch.stack(keypoints, 0)                                   # (B, M, 3)
        batch_idx = torch.arange(batch_size, device=keypoints.device).view(-1, 1).repeat(1, keypoints.shape[1]).view(-1, 1)
        return torch.cat((batch_idx.float(), keypoints.view(-1, 3)), dim=1)

    @staticmethod
    def aggregate_keypoint_features_from_one_source(batch_size, aggregate_func, xyz, xyz_features, xyz_bs_idxs, new_xyz, new_xyz_batch_cnt,
                                                    **kwargs):
        xyz_batch_cnt, contiguous = _counts(xyz_bs_idxs, batch_size)
        if not contiguous:          # the stack query needs batch-contiguous rows: a stable sort keeps each sample's order
            order = torch.argsort(xyz_bs_idxs.long(), stable=True)
            xyz = xyz[order]
            xyz_features = xyz_features[order] if xyz_features is not None else None
        _, pooled = aggregate_func(xyz=xyz.contiguous(), xyz_batch_cnt=xyz_batch_cnt, new_xyz=new_xyz, new_xyz_batch_cnt=new_xyz_batch_cnt,
                                   features=xyz_features.contiguous() if xyz_features is not None else None)
        return pooled

    def forward(self, batch_dict):
        keypoints = self.get_sampled_points(batch_dict)
        batch_size = batch_dict["batch_size"]
        point_features_list = []
        if "bev" in self.model_cfg.FEATURES_SOURCE:
            point_features_list.append(self.interpolate_from_bev_features(keypoints, batch_dict["spatial_features"], batch_size,
                                                                          bev_stride=batch_dict["spatial_features_stride"]))
        new_xyz = keypoints[:, 1:4].contiguous()
        new_xyz_batch_cnt = [self.model_cfg.NUM_KEYPOINTS] * batch_size
        if "raw_points" in self.model_cfg.FEATURES_SOURCE:
            raw_points = batch_dict["points"]
            point_features_list.append(self.aggregate_keypoint_features_from_one_source(
                batch_size=batch_size, aggregate_func=self.SA_rawpoints, xyz=raw_points[:, 1:4],
                xyz_features=raw_points[:, 4:].contiguous() if raw_points.shape[1] > 4 else None, xyz_bs_idxs=raw_points[:, 0],
                new_xyz=new_xyz, new_xyz_batch_cnt=new_xyz_batch_cnt))
        for k, src_name in enumerate(self.SA_layer_names):
            sp = batch_dict["multi_scale_3d_features"][src_name]
            cur_coords = sp.indices
            xyz = common_utils.get_voxel_centers(cur_coords[:, 1:4], downsample_times=self.downsample_times_map[src_name],
                                                 voxel_size=self.voxel_size, point_cloud_range=self.point_cloud_range)
            point_features_list.append(self.aggregate_keypoint_features_from_one_source(
                batch_size=batch_size, aggregate_func=self.SA_layers[k], xyz=xyz.contiguous(), xyz_features=sp.features.contiguous(),
                xyz_bs_idxs=cur_coords[:, 0], new_xyz=new_xyz, new_xyz_batch_cnt=new_xyz_batch_cnt))
        point_features = torch.cat(point_features_list, dim=-1)
        batch_dict["point_features_before_fusion"] = point_features.view(-1, point_features.shape[-1])
        fused = self.vsa_point_feature_fusion[0](point_features.view(-1, point_features.shape[-1]))
        bn = self.vsa_point_feature_fusion[1]
        if ops.bn_rows_supported(fused, bn):
            fused = ops.bn_rows(fused, bn, relu=True)
        else:
            fused = self.vsa_point_feature_fusion[2](bn(fused))
        batch_dict["point_features"] = fused
        batch_dict["point_coords"] = keypoints
        return batch_dict
