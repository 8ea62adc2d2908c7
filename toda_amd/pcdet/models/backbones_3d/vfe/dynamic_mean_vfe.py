"""DynamicMeanVFE (reference pcdet/models/backbones_3d/vfe/dynamic_mean_vfe.py:14-76): the mean of every in-range point of each
voxel, no caps.  On the GPU: ops.dyn_voxel_index + ops.dyn_points_mean (csrc/dynvox.hip, summed in each voxel's point order,
bit-reproducible); on a CPU tensor: torch.unique + index_add_."""
import torch

from toda_amd import ops
from .dynamic_pillar_vfe import torch_dyn_index
from .vfe_template import VFETemplate


class DynamicMeanVFE(VFETemplate):
    def __init__(self, model_cfg, num_point_features, voxel_size, grid_size, point_cloud_range, **kwargs):
        super().__init__(model_cfg=model_cfg)
        self.num_point_features = num_point_features
        self.voxel_size = [float(v) for v in voxel_size]
        self.point_cloud_range = [float(v) for v in point_cloud_range]
        self.grid_size = [int(v) for v in grid_size]

    def get_output_feature_dim(self):
        return self.num_point_features

    def index_points(self, batch_dict):
        """The voxel index of the batch's points, stored in the batch with voxel_coords (see DynamicPillarVFE.index_points): the
        sparse backbone's plan() can then build its rulebooks before the forward."""
        idx = ops.dyn_voxel_index(batch_dict["points"], self.point_cloud_range, self.voxel_size, int(batch_dict["batch_size"]), pillar=False)
        batch_dict["dyn_voxel_index"] = idx
        batch_dict["voxel_coords"] = idx.coords
        return idx

    @torch.no_grad()
    def forward(self, batch_dict, **kwargs):
        points = batch_dict["points"]      # (batch_idx, x, y, z, i, e)
        if not points.is_cuda:
            keep, inv, _cnt, coords, _cell = torch_dyn_index(points, self.point_cloud_range, self.voxel_size, self.grid_size,
                                                             int(batch_dict["batch_size"]), pillar=False)
            data = points[keep, 1:]
            m = coords.shape[0]
            cnt = torch.bincount(inv, minlength=m).to(data.dtype).view(-1, 1)
            batch_dict["voxel_features"] = data.new_zeros((m, data.shape[1])).index_add_(0, inv, data) / cnt
            batch_dict["voxel_coords"] = coords
            return batch_dict
        idx = batch_dict.get("dyn_voxel_index")
        if idx is None:
            idx = self.index_points(batch_dict)
        batch_dict["voxel_features"] = ops.dyn_points_mean(points, idx, 1)
        batch_dict["voxel_coords"] = idx.coords
        return batch_dict
