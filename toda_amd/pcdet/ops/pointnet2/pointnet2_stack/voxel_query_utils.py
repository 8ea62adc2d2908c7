"""Voxel query of the voxel RoI grid pool (reference pcdet/ops/pointnet2/pointnet2_stack/voxel_query_utils.py:10-103).

On CUDA tensors the query runs as one HIP launch per level (ops.voxel_query) over the level's grid index; on CPU tensors the
plain-torch restatement voxel_query_torch below runs instead.  Both return rows of the level's feature table: the reference's
batch-local index plus the first row of the grid point's sample (what its grouping_operation reads)."""
from dataclasses import dataclass

import numpy as np
import torch
import torch.nn as nn

from toda_amd import ops


@dataclass
class VoxelLevel:
    """One sparse level as the pool sees it: coordinates [N, 4] int32 (b, z, y, x), the lattice (Z, Y, X), the batch size and the
    GridIndex of the set (None on CPU tensors, or where no layer has built one yet)."""
    indices: torch.Tensor
    spatial_shape: list
    batch_size: int
    grid_index: object = None

    def index(self):
        if self.grid_index is None:
            self.grid_index = ops.GridIndex.from_coords(self.indices.contiguous(), self.batch_size, self.spatial_shape)
        return self.grid_index


def voxel_query_torch(new_xyz, new_coords, xyz, level, radius, query_range, nsample, chunk=16384):
    """The scan of voxel_query_gpu.cu:10-91 restated in torch: for every grid point the lattice neighbours in dz, dy, dx order
    ((z, y, x) ranges as the reference unpacks QUERY_RANGES), off-lattice and unoccupied ones skipped, dist2 = dx^2 + dy^2 + dz^2
    in fp32 against radius^2 (radius rounded to fp32 first), the first nsample hits in scan order, the first hit filling the
    remaining slots.  Returns (idx [M, nsample] int32 rows, zeros for an empty ball; empty [M] bool)."""
    dev = new_xyz.device
    zr, yr, xr = (int(r) for r in query_range)
    Z, Y, X = (int(v) for v in level.spatial_shape)
    B = int(level.batch_size)
    coords = level.indices.long()
    keys = ((coords[:, 0] * Z + coords[:, 1]) * Y + coords[:, 2]) * X + coords[:, 3]
    skeys, order = torch.sort(keys)
    dz, dy, dx = torch.meshgrid(torch.arange(-zr, zr + 1, device=dev), torch.arange(-yr, yr + 1, device=dev),
                                torch.arange(-xr, xr + 1, device=dev), indexing="ij")
    offs = torch.stack([dz.reshape(-1), dy.reshape(-1), dx.reshape(-1)], dim=1)        # scan order: dz, then dy, then dx
    r32 = np.float32(radius)
    radius2 = float(r32 * r32)
    m_total = new_coords.shape[0]
    idx_all = torch.zeros((m_total, int(nsample)), dtype=torch.int32, device=dev)
    empty_all = torch.ones((m_total,), dtype=torch.bool, device=dev)
    for m0 in range(0, m_total, chunk):
        nc = new_coords[m0:m0 + chunk].long()
        nx = new_xyz[m0:m0 + chunk].float()            # the reference's kernel decides in fp32 whatever the features' dtype
        b = nc[:, 0:1]
        z, y, x = nc[:, 1:2] + offs[:, 0], nc[:, 2:3] + offs[:, 1], nc[:, 3:4] + offs[:, 2]
        on = (b >= 0) & (b < B) & (z >= 0) & (z < Z) & (y >= 0) & (y < Y) & (x >= 0) & (x < X)
        key = ((b * Z + z) * Y + y) * X + x
        pos = torch.searchsorted(skeys, key.clamp(min=0)).clamp(max=max(skeys.shape[0] - 1, 0))
        if skeys.shape[0] == 0:
            continue
        occ = on & (skeys[pos] == key)
        rows = torch.where(occ, order[pos], torch.zeros_like(pos))
        v = xyz.float()[rows]
        ex, ey, ez = v[..., 0] - nx[:, 0:1], v[..., 1] - nx[:, 1:2], v[..., 2] - nx[:, 2:3]
        dist2 = ex * ex + ey * ey + ez * ez
        hit = occ & (dist2 <= radius2)
        rank = torch.cumsum(hit.int(), dim=1) - 1
        cnt = hit.sum(dim=1)
        first = rows.gather(1, hit.int().argmax(dim=1, keepdim=True))
        idx = first.expand(-1, int(nsample)).clone()
        mi, ki = torch.nonzero(hit & (rank < int(nsample)), as_tuple=True)
        idx[mi, rank[mi, ki]] = rows[mi, ki]
        empty = cnt == 0
        idx[empty] = 0
        idx_all[m0:m0 + chunk] = idx.int()
        empty_all[m0:m0 + chunk] = empty
    return idx_all, empty_all


class VoxelQueryAndGrouping(nn.Module):
    def __init__(self, max_range, radius, nsample):
        """max_range: (z, y, x) query ranges in voxels, radius: ball radius, nsample: neighbours per grid point."""
        super().__init__()
        self.max_range, self.radius, self.nsample = max_range, radius, nsample

    def query(self, new_coords, xyz, new_xyz, level):
        """new_coords [M, 4] int32 (b, z, y, x) -> (idx [M, nsample] int32 rows of the level, empty [M] bool)."""
        if new_xyz.is_cuda:
            return ops.voxel_query(new_xyz, new_coords, xyz, level.index(), self.radius, self.max_range, self.nsample)
        return voxel_query_torch(new_xyz, new_coords, xyz, level, self.radius, self.max_range, self.nsample)

    def forward(self, new_coords, xyz, xyz_batch_cnt, new_xyz, new_xyz_batch_cnt, features, level):
        """The reference's grouping (voxel_query_utils.py:61-102): grouped_features [M, C, nsample], grouped_xyz [M, 3, nsample]
        and empty_ball_mask [M].  xyz_batch_cnt / new_xyz_batch_cnt are checked as there; the rows already include the batch
        offsets."""
        assert xyz.shape[0] == xyz_batch_cnt.sum(), f"xyz: {tuple(xyz.shape)}, xyz_batch_cnt: {xyz_batch_cnt}"
        assert new_coords.shape[0] == new_xyz_batch_cnt.sum(), f"new_coords: {tuple(new_coords.shape)}, new_xyz_batch_cnt: {new_xyz_batch_cnt}"
        idx, empty = self.query(new_coords, xyz, new_xyz, level)
        rows = idx.long()
        grouped_xyz = xyz[rows].permute(0, 2, 1)
        grouped_features = features[rows].permute(0, 2, 1)
        return grouped_features, grouped_xyz, empty
