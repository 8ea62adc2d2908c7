"""The PointNet++ stack operations PV-RCNN uses (reference pcdet/ops/pointnet2/pointnet2_stack/pointnet2_utils.py): farthest
point sampling, the stacked ball query and QueryAndGroup.  CUDA tensors run the HIP kernels of csrc/pointnet2_stack.hip; CPU
tensors run plain-torch restatements of the reference's kernels (the host tests and fixtures)."""
import torch
import torch.nn as nn

from toda_amd import ops


def fps_torch(xyz, npoint):
    """sampling_gpu.cu:25-140 restated for one sample xyz [N, 3]: first index 0, temp from 1e10, d = dx dx + dy dy + dz dz in fp32.
    Ties follow the kernel's thread layout: thread t = k mod T (T = opt_n_threads(N)) keeps its first maximum, and the block's
    halving tree keeps the lower slot, which prefers the thread whose log2 T bits read backwards are smallest; then the smallest
    k.  Returns [npoint] int64."""
    n = xyz.shape[0]
    t = ops.fps_threads(n)
    bits = t.bit_length() - 1
    k = torch.arange(n, device=xyz.device)
    r = k % t
    rev = torch.zeros_like(r)
    for i in range(bits):
        rev |= ((r >> i) & 1) << (bits - 1 - i)
    rank = rev * n + k
    temp = torch.full((n,), 1e10, dtype=torch.float32, device=xyz.device)
    out = torch.zeros((npoint,), dtype=torch.int64, device=xyz.device)
    old = 0
    for j in range(1, npoint):
        diff = xyz - xyz[old]
        d = diff[:, 0] * diff[:, 0] + diff[:, 1] * diff[:, 1] + diff[:, 2] * diff[:, 2]
        temp = torch.minimum(d, temp)
        tied = temp == temp.max()
        old = int(torch.where(tied, rank, rank.new_full((), 1 << 62)).argmin())
        out[j] = old
    return out


def farthest_point_sample(xyz, npoint):
    """xyz [B, N, 3] -> [B, npoint] int32 (reference FarthestPointSampling.apply)."""
    assert xyz.is_contiguous() and xyz.dim() == 3
    b, n, _ = xyz.shape
    if xyz.is_cuda:
        return ops.farthest_point_sample(xyz.view(-1, 3), [n] * b, npoint)
    return torch.stack([fps_torch(xyz[k], npoint) for k in range(b)], 0).int()


def stack_farthest_point_sample_counts(xyz, counts, npoint):
    """Farthest point sampling of each sample of a batch-contiguous stack xyz [N, 3] with per-sample counts: [B, npoint]
    sample-local int32 indices (one launch for the whole batch on CUDA tensors)."""
    if xyz.is_cuda:
        return ops.farthest_point_sample(xyz, counts, npoint)
    outs, s = [], 0
    for c in counts:
        outs.append(fps_torch(xyz[s:s + c], npoint))
        s += c
    return torch.stack(outs, 0).int()


def ball_query_torch(radius, nsample, xyz, xyz_batch_cnt, new_xyz, new_xyz_batch_cnt):
    """ball_query_gpu.cu:15-64 + BallQuery.forward restated: idx [M, nsample] int32 sample-local indices (zeros for an empty
    ball) and the empty mask."""
    m = new_xyz.shape[0]
    idx = torch.zeros((m, nsample), dtype=torch.int32)
    empty = torch.zeros((m,), dtype=torch.bool)
    r2 = torch.tensor(radius, dtype=torch.float32) * torch.tensor(radius, dtype=torch.float32)
    xs = [0] + torch.cumsum(torch.as_tensor(xyz_batch_cnt).long(), 0).tolist()
    ns_ = [0] + torch.cumsum(torch.as_tensor(new_xyz_batch_cnt).long(), 0).tolist()
    for b in range(len(xs) - 1):
        pts = xyz[xs[b]:xs[b + 1]]
        for q in range(ns_[b], ns_[b + 1]):
            c = new_xyz[q]
            d2 = (c[0] - pts[:, 0]) * (c[0] - pts[:, 0]) + (c[1] - pts[:, 1]) * (c[1] - pts[:, 1]) + (c[2] - pts[:, 2]) * (c[2] - pts[:, 2])
            hits = torch.nonzero(d2 < r2).view(-1)[:nsample]
            if hits.numel() == 0:
                empty[q] = True
                continue
            idx[q, :] = hits[0]
            idx[q, :hits.numel()] = hits
    return idx, empty


def _check_stack(xyz, xyz_batch_cnt, new_xyz, new_xyz_batch_cnt):
    assert xyz.shape[0] == int(sum(int(c) for c in xyz_batch_cnt)), f"xyz: {tuple(xyz.shape)}, xyz_batch_cnt: {xyz_batch_cnt}"
    assert new_xyz.shape[0] == int(sum(int(c) for c in new_xyz_batch_cnt)), \
        f"new_xyz: {tuple(new_xyz.shape)}, new_xyz_batch_cnt: {new_xyz_batch_cnt}"


def ball_query_multi(radii, nsamples, xyz, xyz_batch_cnt, new_xyz, new_xyz_batch_cnt):
    """The ball query of every radius of an MSG layer: [(idx [M, ns] int32 rows of xyz, empty [M] bool)] per radius.  CUDA:
    one scan for all radii (the stacks must be batch-contiguous, as the reference's kernel assumes); CPU: the restatement per
    radius, sample offsets added."""
    if xyz.is_cuda:
        xs = ops.batch_starts(xyz_batch_cnt, xyz.device)
        ns_ = ops.batch_starts(new_xyz_batch_cnt, xyz.device)
        return ops.ball_query_stack(radii, nsamples, xyz, xs, new_xyz, ns_)
    outs = []
    starts = torch.cumsum(torch.as_tensor(xyz_batch_cnt).long(), 0) - torch.as_tensor(xyz_batch_cnt).long()
    which = torch.repeat_interleave(torch.arange(len(new_xyz_batch_cnt)), torch.as_tensor(new_xyz_batch_cnt).long())
    for r, ns in zip(radii, nsamples):
        idx, empty = ball_query_torch(r, ns, xyz, xyz_batch_cnt, new_xyz, new_xyz_batch_cnt)
        idx = (idx.long() + starts[which].unsqueeze(1)).int()
        idx[empty] = 0
        outs.append((idx, empty))
    return outs


def ball_query(radius, nsample, xyz, xyz_batch_cnt, new_xyz, new_xyz_batch_cnt):
    """Reference BallQuery.apply: idx [M, nsample] int32 sample-local indices (0 for empty balls), empty_ball_mask [M]."""
    _check_stack(xyz, xyz_batch_cnt, new_xyz, new_xyz_batch_cnt)
    idx, empty = ball_query_multi([radius], [nsample], xyz, xyz_batch_cnt, new_xyz, new_xyz_batch_cnt)[0]
    counts = torch.as_tensor(xyz_batch_cnt, device=idx.device).long()
    starts = torch.cumsum(counts, 0) - counts
    which = torch.repeat_interleave(torch.arange(len(counts), device=idx.device),
                                    torch.as_tensor(new_xyz_batch_cnt, device=idx.device).long())
    local = (idx.long() - starts[which].unsqueeze(1)).int()
    local[empty] = 0
    return local, empty


class QueryAndGroup(nn.Module):
    """Reference QueryAndGroup (pointnet2_utils.py:116-166): [M, 3 + C, nsample] grouped relative xyz then features, empty
    balls zeroed.  StackSAModuleMSG does not build this tensor on CUDA tensors (it runs ops.sa_gather); this module is the
    reference's composition for the CPU path."""

    def __init__(self, radius, nsample, use_xyz=True):
        super().__init__()
        self.radius, self.nsample, self.use_xyz = radius, nsample, use_xyz

    @staticmethod
    def group(xyz, new_xyz, features, idx, empty, use_xyz=True):
        rows = idx.long()
        grouped_xyz = xyz[rows].permute(0, 2, 1) - new_xyz.unsqueeze(-1)            # (M, 3, nsample)
        grouped_xyz[empty] = 0
        if features is None:
            assert use_xyz, "Cannot have not features and not use xyz as a feature!"
            return grouped_xyz
        grouped_features = features[rows].permute(0, 2, 1).clone()                 # (M, C, nsample)
        grouped_features[empty] = 0
        return torch.cat([grouped_xyz, grouped_features], dim=1) if use_xyz else grouped_features

    def forward(self, xyz, xyz_batch_cnt, new_xyz, new_xyz_batch_cnt, features=None):
        _check_stack(xyz, xyz_batch_cnt, new_xyz, new_xyz_batch_cnt)
        idx, empty = ball_query_multi([self.radius], [self.nsample], xyz, xyz_batch_cnt, new_xyz, new_xyz_batch_cnt)[0]
        return self.group(xyz, new_xyz, features, idx, empty, self.use_xyz), idx
