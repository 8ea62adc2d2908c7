"""DynamicPillarVFE / PFNLayerV2 (reference pcdet/models/backbones_3d/vfe/dynamic_pillar_vfe.py:13-151): every in-range point
is used, grouped by pillar without caps.  On the GPU the grouping, the per-pillar mean, the per-point decoration, the segmented
max and the gather-concat are the HIP kernels of csrc/dynvox.hip (ops.dyn_*): integer atomics only, bit-reproducible.  The
Linear stays a torch matmul, as in PillarVFE; BatchNorm1d + ReLU go through ops.bn_rows where it applies.  On a CPU tensor both
modules run a plain-torch restatement (torch.unique + index_add_ / scatter_reduce) for the CPU plumbing configurations."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from toda_amd import ops
from .vfe_template import VFETemplate


def torch_dyn_index(points, point_cloud_range, voxel_size, grid_size, batch_size, pillar):
    """Plain-torch grouping of dynamic_pillar_vfe.py:101-113 / dynamic_mean_vfe.py:55-66: (keep [N], inv [K], cnt [M],
    coords [M, 4] (b, z, y, x), cell [K, 3] (x, y, z)).  Rows whose batch index is outside [0, batch_size) are dropped, as the
    kernel does."""
    axes = 2 if pillar else 3
    lo = torch.as_tensor([float(v) for v in point_cloud_range[:axes]], dtype=torch.float32, device=points.device)
    vs = torch.as_tensor([float(v) for v in voxel_size[:axes]], dtype=torch.float32, device=points.device)
    grid = [int(v) for v in grid_size]
    f = torch.floor((points[:, 1:1 + axes] - lo) / vs)
    keep = ((f >= 0) & (f < torch.as_tensor(grid[:axes], dtype=torch.float32, device=points.device))).all(dim=1)
    keep &= (points[:, 0] >= 0) & (points[:, 0] < batch_size)
    cell = f[keep].long()
    b = points[keep, 0].long()
    if pillar:
        merge = (b * grid[0] + cell[:, 0]) * grid[1] + cell[:, 1]
    else:
        merge = ((b * grid[0] + cell[:, 0]) * grid[1] + cell[:, 1]) * grid[2] + cell[:, 2]
    unq, inv, cnt = torch.unique(merge, return_inverse=True, return_counts=True)
    if pillar:
        plane = grid[0] * grid[1]
        coords = torch.stack([unq // plane, torch.zeros_like(unq), unq % grid[1], (unq % plane) // grid[1]], dim=1)
    else:
        vol = grid[0] * grid[1] * grid[2]
        coords = torch.stack([unq // vol, unq % grid[2], (unq // grid[2]) % grid[1], (unq % vol) // (grid[1] * grid[2])], dim=1)
    return keep, inv, cnt.int(), coords.int(), cell


class PFNLayerV2(nn.Module):
    def __init__(self, in_channels, out_channels, use_norm=True, last_layer=False):
        super().__init__()
        self.last_vfe = last_layer
        self.use_norm = use_norm
        if not self.last_vfe:
            out_channels = out_channels // 2
        if self.use_norm:
            self.linear = nn.Linear(in_channels, out_channels, bias=False)
            self.norm = nn.BatchNorm1d(out_channels, eps=1e-3, momentum=0.01)
        else:
            self.linear = nn.Linear(in_channels, out_channels, bias=True)
        self.relu = nn.ReLU()

    def forward(self, inputs, index):
        """inputs [K, C_in]; index: an ops.DynVoxelIndex (GPU) or (unq_inv, M) (CPU restatement)."""
        x = self.linear(inputs)
        if isinstance(index, ops.DynVoxelIndex):
            if self.use_norm and ops.bn_rows_supported(x, self.norm):
                x = ops.bn_rows(x, self.norm, True)
            else:
                x = self.relu(self.norm(x) if self.use_norm else x)
            x_max = ops.dyn_seg_max(x, index)[0]
            return x_max if self.last_vfe else ops.dyn_gather_concat(x, x_max, index)
        inv, m = index
        x = self.relu(self.norm(x) if self.use_norm else x)
        x_max = x.new_zeros((m, x.shape[1])).scatter_reduce(0, inv.view(-1, 1).expand_as(x), x, "amax", include_self=False)
        return x_max if self.last_vfe else torch.cat([x, x_max[inv, :]], dim=1)


class DynamicPillarVFE(VFETemplate):
    def __init__(self, model_cfg, num_point_features, voxel_size, grid_size, point_cloud_range, **kwargs):
        super().__init__(model_cfg=model_cfg)
        self.use_norm = self.model_cfg.USE_NORM
        self.with_distance = self.model_cfg.WITH_DISTANCE
        self.use_absolute_xyz = self.model_cfg.USE_ABSLOTE_XYZ
        num_point_features += 6 if self.use_absolute_xyz else 3
        if self.with_distance:
            num_point_features += 1
        self.num_filters = list(self.model_cfg.NUM_FILTERS)
        assert len(self.num_filters) > 0
        dims = [num_point_features] + self.num_filters
        self.pfn_layers = nn.ModuleList(
            PFNLayerV2(dims[i], dims[i + 1], self.use_norm, last_layer=(i >= len(dims) - 2)) for i in range(len(dims) - 1)
        )
        self.voxel_size = [float(v) for v in voxel_size]
        self.point_cloud_range = [float(v) for v in point_cloud_range]
        self.grid_size = [int(v) for v in grid_size]
        self.voxel_x, self.voxel_y, self.voxel_z = self.voxel_size
        self.x_offset = self.voxel_x / 2 + self.point_cloud_range[0]
        self.y_offset = self.voxel_y / 2 + self.point_cloud_range[1]
        self.z_offset = self.voxel_z / 2 + self.point_cloud_range[2]

    def get_output_feature_dim(self):
        return self.num_filters[-1]

    def index_points(self, batch_dict):
        """Build the pillar index of the batch's points (ops.dyn_voxel_index, one host read) and store it in the batch together with
        voxel_coords: called by prepare_batch_on_gpu on the input pipeline's side stream, or by forward when the batch has none."""
        idx = ops.dyn_voxel_index(batch_dict["points"], self.point_cloud_range, self.voxel_size, int(batch_dict["batch_size"]), pillar=True)
        batch_dict["dyn_voxel_index"] = idx
        batch_dict["voxel_coords"] = idx.coords
        return idx

    def forward(self, batch_dict, **kwargs):
        points = batch_dict["points"]      # (batch_idx, x, y, z, i, e)
        if not points.is_cuda:
            return self._forward_torch(batch_dict)
        idx = batch_dict.get("dyn_voxel_index")
        if idx is None:
            idx = self.index_points(batch_dict)
        mean = ops.dyn_points_mean(points, idx, 1, 3)
        features = ops.dyn_pillar_decorate(points, idx, mean, self.voxel_size, [self.x_offset, self.y_offset, self.z_offset],
                                           self.use_absolute_xyz, self.with_distance)
        for pfn in self.pfn_layers:
            features = pfn(features, idx)
        batch_dict["pillar_features"] = features
        batch_dict["voxel_coords"] = idx.coords
        return batch_dict

    def decorate_torch(self, points, keep, inv, cell, m):
        """dynamic_pillar_vfe.py:110-129 in plain torch: the rows the first Linear reads."""
        points = points[keep]
        xyz = points[:, 1:4]
        cnt = torch.bincount(inv, minlength=m).to(points.dtype).view(-1, 1)
        mean = xyz.new_zeros((m, 3)).index_add_(0, inv, xyz) / cnt
        f_cluster = xyz - mean[inv, :]
        f_center = torch.stack([xyz[:, 0] - (cell[:, 0].to(xyz.dtype) * self.voxel_x + self.x_offset),
                                xyz[:, 1] - (cell[:, 1].to(xyz.dtype) * self.voxel_y + self.y_offset),
                                xyz[:, 2] - self.z_offset], dim=1)
        parts = [points[:, 1:] if self.use_absolute_xyz else points[:, 4:], f_cluster, f_center]
        if self.with_distance:
            parts.append(torch.norm(xyz, 2, dim=1, keepdim=True))
        return torch.cat(parts, dim=-1)

    def _forward_torch(self, batch_dict):
        points = batch_dict["points"]
        keep, inv, _cnt, coords, cell = torch_dyn_index(points, self.point_cloud_range, self.voxel_size, self.grid_size,
                                                        int(batch_dict["batch_size"]), pillar=True)
        m = coords.shape[0]
        features = self.decorate_torch(points, keep, inv, cell, m)
        for pfn in self.pfn_layers:
            features = pfn(features, (inv, m))
        batch_dict["pillar_features"] = features
        batch_dict["voxel_coords"] = coords
        return batch_dict
