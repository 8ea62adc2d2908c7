"""NeighborVoxelSAModuleMSG (reference pcdet/ops/pointnet2/pointnet2_stack/voxel_pool_modules.py:8-131): the voxel RoI grid pool
of one level, with the reference's module tree (groupers, mlps_in.k.{0,1}, mlps_pos.k.{0,1}, mlps_out.k.{0,1}).

CUDA tensors: mlps_in and mlps_out run as row matmuls + ops.bn_rows; the grouping, mlps_pos, sum, ReLU and max pool are one
fused HIP pass (ops.voxel_neighbor_pool) with mlps_pos folded into an affine map of the relative position d: the BatchNorm2d
statistics of Conv2d(d) are W mu and W^T Sigma W (mu, Sigma: moments of d, ops.voxel_pool_moments) in training, the running
statistics in eval.  CPU tensors: the plain-torch restatement of the reference's composition (pool_torch)."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from toda_amd import ops

from . import voxel_query_utils


def pool_torch(features_in, idx, empty, xyz, new_xyz, mlp_pos, pool_method="max_pool"):
    """The reference's composition (voxel_pool_modules.py:96-125) on [M, C, nsample] tensors: grouped features and relative
    positions (zeroed for empty balls), Conv2d + BatchNorm2d of the positions, the sum, ReLU, max pool -> [M, C]."""
    rows = idx.long()
    grouped_features = features_in[rows].permute(0, 2, 1).clone()          # (M, C, nsample)
    grouped_features[empty] = 0
    grouped_features = grouped_features.permute(1, 0, 2).unsqueeze(dim=0)   # (1, C, M, nsample)
    grouped_xyz = xyz[rows].permute(0, 2, 1) - new_xyz.unsqueeze(-1)       # (M, 3, nsample)
    grouped_xyz[empty] = 0
    grouped_xyz = grouped_xyz.permute(1, 0, 2).unsqueeze(0)
    new_features = torch.relu(grouped_features + mlp_pos(grouped_xyz))
    if pool_method != "max_pool":
        raise NotImplementedError(f"POOL_METHOD {pool_method}")
    new_features = F.max_pool2d(new_features, kernel_size=[1, new_features.size(3)]).squeeze(dim=-1)     # (1, C, M)
    return new_features.squeeze(dim=0).permute(1, 0)


def folded_position_map(mlp_pos, idx, empty, xyz, new_xyz):
    """mlps_pos = [Conv2d(3 -> C, 1 x 1, no bias), BatchNorm2d(C)] on d as a per-channel affine map a [C, 3] . d + b [C],
    differentiable in the Conv2d weight and the BatchNorm2d affine parameters.  Training: batch statistics W mu / W^T Sigma W over
    the M x nsample entries, running statistics updated as nn.BatchNorm2d does (unbiased variance, n = M x nsample); eval: the
    running statistics."""
    conv, bn = mlp_pos[0], mlp_pos[1]
    w = conv.weight.view(conv.out_channels, 3)
    training = bn.training or not bn.track_running_stats
    if training:
        mu, cov = ops.voxel_pool_moments(idx, empty, xyz, new_xyz)
        mean = w @ mu.float()
        var = ((w @ cov.float()) * w).sum(dim=1)
        if bn.training and bn.track_running_stats:
            n = idx.numel()
            if bn.momentum is None:
                bn.num_batches_tracked.add_(1)
                factor = 1.0 / bn.num_batches_tracked.float()
            else:
                ops.bump_bn_counter(bn)
                factor = bn.momentum
            with torch.no_grad():
                bn.running_mean.mul_(1 - factor).add_(factor * mean.detach())
                bn.running_var.mul_(1 - factor).add_(factor * var.detach() * (n / max(n - 1, 1)))
    else:
        mean, var = bn.running_mean, bn.running_var
    inv = torch.rsqrt(var + bn.eps)
    gamma = bn.weight if bn.weight is not None else torch.ones_like(inv)
    beta = bn.bias if bn.bias is not None else torch.zeros_like(inv)
    a = (gamma * inv).unsqueeze(1) * w
    b = beta - gamma * mean * inv
    return a, b


class NeighborVoxelSAModuleMSG(nn.Module):
    def __init__(self, *, query_ranges, radii, nsamples, mlps, use_xyz=True, pool_method="max_pool"):
        """query_ranges: (z, y, x) voxel ranges per scale, radii / nsamples: ball radius and size per scale, mlps: [C_in, C_mid,
        C_out] per scale, pool_method: max_pool (avg_pool is accepted by the reference but used by no config: refused)."""
        super().__init__()
        assert len(query_ranges) == len(nsamples) == len(mlps)
        if pool_method != "max_pool":
            raise NotImplementedError(f"NeighborVoxelSAModuleMSG pool_method {pool_method}: only max_pool is on this path")
        self.groupers = nn.ModuleList()
        self.mlps_in = nn.ModuleList()
        self.mlps_pos = nn.ModuleList()
        self.mlps_out = nn.ModuleList()
        for i in range(len(query_ranges)):
            self.groupers.append(voxel_query_utils.VoxelQueryAndGrouping(query_ranges[i], radii[i], nsamples[i]))
            spec = mlps[i]
            self.mlps_in.append(nn.Sequential(nn.Conv1d(spec[0], spec[1], kernel_size=1, bias=False), nn.BatchNorm1d(spec[1])))
            self.mlps_pos.append(nn.Sequential(nn.Conv2d(3, spec[1], kernel_size=1, bias=False), nn.BatchNorm2d(spec[1])))
            self.mlps_out.append(nn.Sequential(nn.Conv1d(spec[1], spec[2], kernel_size=1, bias=False), nn.BatchNorm1d(spec[2]), nn.ReLU()))
        self.relu = nn.ReLU()
        self.pool_method = pool_method
        self.init_weights()

    def init_weights(self):
        for m in self.modules():
            if isinstance(m, (nn.Conv2d, nn.Conv1d)):
                nn.init.kaiming_normal_(m.weight)
                if m.bias is not None:
                    nn.init.constant_(m.bias, 0)
            if isinstance(m, (nn.BatchNorm2d, nn.BatchNorm1d)):
                nn.init.constant_(m.weight, 1.0)
                nn.init.constant_(m.bias, 0)

    def forward(self, xyz, xyz_batch_cnt, new_xyz, new_xyz_batch_cnt, new_coords, features, level):
        """xyz [N, 3] voxel centres of the level's rows, new_xyz [M, 3] grid points, new_coords [M, 4] int32 in the reference's
        (b, x, y, z) order, features [N, C_in], level: voxel_query_utils.VoxelLevel of the rows (in place of the reference's
        dense voxel2point table).  xyz_batch_cnt / new_xyz_batch_cnt are accepted for the reference's signature and not read:
        the query's rows already carry the batch offsets.  Returns [M, sum of C_out]."""
        from ....models.roi_heads.second_head import run_fc_rows

        new_coords = new_coords[:, [0, 3, 2, 1]].contiguous()
        out = []
        for k in range(len(self.groupers)):
            grouper = self.groupers[k]
            if features.is_cuda:
                features_in = run_fc_rows(self.mlps_in[k], features)
                idx, empty = grouper.query(new_coords, xyz, new_xyz, level)
                a, b = folded_position_map(self.mlps_pos[k], idx, empty, xyz, new_xyz)
                pooled = ops.voxel_neighbor_pool(features_in, a, b, idx, empty, xyz, new_xyz)
                out.append(run_fc_rows(self.mlps_out[k], pooled))
            else:
                features_in = self.mlps_in[k](features.permute(1, 0).unsqueeze(0)).squeeze(0).permute(1, 0)
                idx, empty = grouper.query(new_coords, xyz, new_xyz, level)
                pooled = pool_torch(features_in, idx, empty, xyz, new_xyz, self.mlps_pos[k], self.pool_method)
                out.append(self.mlps_out[k](pooled.permute(1, 0).unsqueeze(0)).squeeze(0).permute(1, 0))
        return torch.cat(out, dim=1)
