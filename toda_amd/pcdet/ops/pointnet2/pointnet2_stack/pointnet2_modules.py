"""StackSAModuleMSG with max_pool (reference pcdet/ops/pointnet2/pointnet2_stack/pointnet2_modules.py:10-120), with the
reference's module tree (groupers, mlps.k.{0,1,2,...}: Conv2d 1 x 1 no bias, BatchNorm2d, ReLU per layer).

CUDA tensors: one ball-query scan fills every radius's table; layer 1 projects the source rows first (P = F W_f^T, one GEMM on N
rows) and gathers z1 = P[idx] + W_d d per entry (ops.sa_gather); the later layers run on the [M x nsample, C] rows with
ops.bn_rows (BatchNorm2d's training statistics over all M x nsample entries and its running-statistics update) and GEMMs; a HIP
max over nsample ends the branch (ops.sa_max).  CPU tensors: the reference's composition on [1, C, M, nsample] tensors."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from toda_amd import ops

from . import pointnet2_utils


def build_local_aggregation_module(input_channels, config):
    name = config.get("NAME", "StackSAModuleMSG")
    if name != "StackSAModuleMSG":
        raise NotImplementedError(f"local aggregation {name}: only StackSAModuleMSG is on this path (PV-RCNN++ is out of scope)")
    mlps = [[input_channels] + list(m) for m in config.MLPS]
    layer = StackSAModuleMSG(radii=config.POOL_RADIUS, nsamples=config.NSAMPLE, mlps=mlps, use_xyz=True,
                             pool_method=config.get("POOL_METHOD", "max_pool"))
    return layer, sum(m[-1] for m in mlps)


def _bn_rows_2d(x, bn, relu):
    """BatchNorm2d (+ ReLU) of [1, C, M, ns] applied to its [M ns, C] rows: the same statistics as nn.BatchNorm2d (n = M ns).
    ops.bn_rows where it covers the module (plain BatchNorm2d, its channel counts); any other norm (SyncBatchNorm under
    --sync_bn) runs as itself on the [1, C, M ns, 1] view."""
    c = x.shape[1]
    if type(bn) is nn.BatchNorm2d and 4 <= c <= 128 and 256 % c == 0 and bn.affine and bn.momentum is not None and x.shape[0] > 1:
        return ops.bn_rows(x, bn, relu=relu)
    y = bn(x.t().unsqueeze(0).unsqueeze(-1)).squeeze(-1).squeeze(0).t()
    return torch.relu(y) if relu else y


class StackSAModuleMSG(nn.Module):
    def __init__(self, *, radii, nsamples, mlps, use_xyz=True, pool_method="max_pool"):
        super().__init__()
        assert len(radii) == len(nsamples) == len(mlps)
        if pool_method != "max_pool":
            raise NotImplementedError(f"StackSAModuleMSG pool_method {pool_method}: only max_pool is on this path")
        if not use_xyz:
            raise NotImplementedError("StackSAModuleMSG: use_xyz=False is used by no PV-RCNN config")
        self.radii, self.nsamples = list(radii), list(nsamples)
        self.groupers = nn.ModuleList()
        self.mlps = nn.ModuleList()
        for i in range(len(radii)):
            self.groupers.append(pointnet2_utils.QueryAndGroup(radii[i], nsamples[i], use_xyz=use_xyz))
            spec = list(mlps[i])
            spec[0] += 3
            layers = []
            for k in range(len(spec) - 1):
                layers += [nn.Conv2d(spec[k], spec[k + 1], kernel_size=1, bias=False), nn.BatchNorm2d(spec[k + 1]), nn.ReLU()]
            self.mlps.append(nn.Sequential(*layers))
        self.pool_method = pool_method
        self.init_weights()

    def init_weights(self):
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight)
                if m.bias is not None:
                    nn.init.constant_(m.bias, 0)
            if isinstance(m, nn.BatchNorm2d):
                nn.init.constant_(m.weight, 1.0)
                nn.init.constant_(m.bias, 0)

    def _branch_rows(self, k, features, xyz, new_xyz, idx, empty):
        """mlps[k] + max pool over the rows layout (CUDA)."""
        mods = list(self.mlps[k])
        m, ns = idx.shape
        w1 = mods[0].weight.view(mods[0].out_channels, mods[0].in_channels)
        if features is not None and features.shape[1] > 0:
            proj = features @ w1[:, 3:].t()
        else:
            proj = xyz.new_zeros((xyz.shape[0], w1.shape[0]))
        z = ops.sa_gather(proj, w1[:, :3], idx, empty, xyz, new_xyz)
        z = _bn_rows_2d(z, mods[1], relu=True)
        for j in range(3, len(mods), 3):
            conv, bn = mods[j], mods[j + 1]
            z = _bn_rows_2d(F.linear(z, conv.weight.view(conv.out_channels, conv.in_channels)), bn, relu=True)
        return ops.sa_max(z, m, ns)

    def forward(self, xyz, xyz_batch_cnt, new_xyz, new_xyz_batch_cnt, features=None, empty_voxel_set_zeros=True):
        """xyz [N, 3], new_xyz [M, 3] batch-contiguous, *_batch_cnt per-sample counts, features [N, C] -> (new_xyz, [M, sum C_out])."""
        pointnet2_utils._check_stack(xyz, xyz_batch_cnt, new_xyz, new_xyz_batch_cnt)
        tables = pointnet2_utils.ball_query_multi(self.radii, self.nsamples, xyz, xyz_batch_cnt, new_xyz, new_xyz_batch_cnt)
        out = []
        for k, (idx, empty) in enumerate(tables):
            if xyz.is_cuda:
                out.append(self._branch_rows(k, features, xyz.contiguous(), new_xyz.contiguous(), idx, empty))
                continue
            grouped = pointnet2_utils.QueryAndGroup.group(xyz, new_xyz, features, idx, empty, True)      # (M, 3 + C, ns)
            grouped = grouped.permute(1, 0, 2).unsqueeze(dim=0)
            grouped = self.mlps[k](grouped)
            pooled = F.max_pool2d(grouped, kernel_size=[1, grouped.size(3)]).squeeze(dim=-1)
            out.append(pooled.squeeze(dim=0).permute(1, 0))
        return new_xyz, torch.cat(out, dim=1)
