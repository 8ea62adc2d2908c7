#!/usr/bin/env python
"""Capture golden vectors from the REFERENCE's Voxel R-CNN RoI head (build container only, CPU).

    python tests/golden/capture_voxel_rcnn.py
writes tests/golden/voxel_rcnn_query.npz (the voxel query of a small level), voxel_rcnn_head.npz (a small VoxelRCNNHead: state
dict, eval-mode batch_cls_preds / batch_box_preds, train-mode loss terms and gradients with DP_RATIO 0) and
voxel_rcnn_corner.npz (loss_utils.get_corner_loss_lidar).

pcdet/models/roi_heads/voxelrcnn_head.py, roi_head_template.py, target_assigner/proposal_target_layer.py and
ops/pointnet2/pointnet2_stack/{voxel_query_utils,voxel_pool_modules,pointnet2_utils}.py are loaded by path
(capture_second_head.setup()).  Their compiled helper pointnet2_stack_cuda cannot be built in this image, so its
voxel_query_wrapper and group_points_wrapper / group_points_grad_wrapper are served by numpy / torch stand-ins written from
src/voxel_query_gpu.cu and src/group_points_gpu.cu, and torch.cuda.IntTensor / FloatTensor allocate on the host.  The query
indices in these fixtures are therefore self-referential: what they pin is the reference's Python logic - the grid points and
their `//` coordinates, the batch offsets subtracted from the query and added back by the grouping, the empty-ball masks, the
layer order, the pooled [R, G^3, sum C] layout, the box decoding and the losses.  No candidate's dist2 lies within 1e-5
(relative) of radius^2, and in training no pooled maximum lies within 1e-5 of the best value of another voxel or of 0 (both
asserted below), so last-bit differences of a device evaluation cannot flip a neighbour or an arg-max.  The IoUs of the roi
sampler come from the oracle as in capture_second_head.py, with the same margin check on its thresholds.
Only inputs, parameters, seeds and outputs are stored - no reference source.
"""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import capture_reference as CR  # noqa: E402
import capture_second_head as CS  # noqa: E402
from capture_reference import EasyDict  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
PC_RANGE = [-24.0, -24.0, -3.0, 24.0, 24.0, 1.0]
VOXEL = [0.4, 0.4, 0.5]
LEVELS = (("x_conv2", 2, 6, 0.9, [2, 2, 2]), ("x_conv3", 4, 8, 1.7, [2, 2, 1]))    # name, stride, channels, radius, (z, y, x) ranges
GRID = 3
NSAMPLE = 8
TRACE = {"dist2_margin": np.inf, "pool": None}


def head_cfg():
    layers = {name: dict(MLPS=[[4, 4]], QUERY_RANGES=[rng], POOL_RADIUS=[r], NSAMPLE=[NSAMPLE], POOL_METHOD="max_pool")
              for name, _, _, r, rng in LEVELS}
    return EasyDict(dict(
        NAME="VoxelRCNNHead", CLASS_AGNOSTIC=True, SHARED_FC=[16, 16], CLS_FC=[16, 16], REG_FC=[16, 16], DP_RATIO=0.0,
        NMS_CONFIG=dict(TRAIN=dict(NMS_TYPE="nms_gpu", MULTI_CLASSES_NMS=False, NMS_PRE_MAXSIZE=9000, NMS_POST_MAXSIZE=512, NMS_THRESH=0.8),
                        TEST=dict(NMS_TYPE="nms_gpu", MULTI_CLASSES_NMS=False, NMS_PRE_MAXSIZE=1024, NMS_POST_MAXSIZE=100, NMS_THRESH=0.7)),
        ROI_GRID_POOL=dict(FEATURES_SOURCE=[n for n, *_ in LEVELS], PRE_MLP=True, GRID_SIZE=GRID, POOL_LAYERS=layers),
        TARGET_CONFIG=CS.TARGET_CONFIG,
        LOSS_CONFIG=dict(CLS_LOSS="BinaryCrossEntropy", REG_LOSS="smooth-l1", CORNER_LOSS_REGULARIZATION=True,
                         LOSS_WEIGHTS=dict(rcnn_cls_weight=1.0, rcnn_reg_weight=1.0, rcnn_corner_weight=1.0, code_weights=[1.0] * 7))))


def voxel_query_wrapper(M, R1, R2, R3, nsample, radius, z_range, y_range, x_range, new_xyz, xyz, new_coords, point_indices, idx):
    """voxel_query_gpu.cu:10-91 in numpy fp32 (dist2 summed in the kernel's order); records how close any candidate comes to
    the radius."""
    nx, vx = new_xyz.numpy(), xyz.numpy()
    nc, table, out = new_coords.numpy(), point_indices.numpy(), idx.numpy()
    r2 = np.float32(radius) * np.float32(radius)
    for m in range(M):
        b, cz, cy, cx = (int(v) for v in nc[m])
        cnt = 0
        for dz in range(-z_range, z_range + 1):
            z = cz + dz
            if z < 0 or z >= R1:
                continue
            for dy in range(-y_range, y_range + 1):
                y = cy + dy
                if y < 0 or y >= R2:
                    continue
                for dx in range(-x_range, x_range + 1):
                    x = cx + dx
                    if x < 0 or x >= R3:
                        continue
                    n = int(table[b, z, y, x])
                    if n < 0:
                        continue
                    d = vx[n] - nx[m]
                    dist2 = np.float32(np.float32(d[0] * d[0]) + np.float32(d[1] * d[1])) + np.float32(d[2] * d[2])
                    TRACE["dist2_margin"] = min(TRACE["dist2_margin"], abs(float(dist2) - float(r2)) / float(r2))
                    if dist2 > r2:
                        continue
                    if cnt < nsample:
                        if cnt == 0:
                            out[m, :] = n
                        out[m, cnt] = n
                        cnt += 1
        if cnt == 0:
            out[m, 0] = -1


def _starts(cnt):
    return torch.cat([torch.zeros(1, dtype=torch.long), torch.cumsum(cnt.long(), 0)[:-1]])


def group_points_wrapper(B, M, C, nsample, features, features_batch_cnt, idx, idx_batch_cnt, output):
    """group_points_gpu.cu: output[m, c, s] = features[first row of m's sample + idx[m, s], c]."""
    start = _starts(features_batch_cnt).repeat_interleave(idx_batch_cnt.long())
    output.copy_(features[start.unsqueeze(1) + idx.long()].permute(0, 2, 1))


def group_points_grad_wrapper(B, M, C, N, nsample, grad_out, idx, idx_batch_cnt, features_batch_cnt, grad_features):
    start = _starts(features_batch_cnt).repeat_interleave(idx_batch_cnt.long())
    rows = (start.unsqueeze(1) + idx.long()).reshape(-1)
    grad_features.index_add_(0, rows, grad_out.permute(0, 2, 1).reshape(-1, C))


def setup():
    M = CS.setup()
    A = CR.ALIAS
    for name in (f"{A}.ops.pointnet2", f"{A}.ops.pointnet2.pointnet2_stack"):
        CR._pkg(name)
    stub = f"{A}.ops.pointnet2.pointnet2_stack.pointnet2_stack_cuda"
    cu = types.ModuleType(stub)
    cu.voxel_query_wrapper = voxel_query_wrapper
    cu.group_points_wrapper = group_points_wrapper
    cu.group_points_grad_wrapper = group_points_grad_wrapper
    sys.modules[stub] = cu
    setattr(sys.modules[f"{A}.ops.pointnet2.pointnet2_stack"], "pointnet2_stack_cuda", cu)
    torch.cuda.IntTensor = lambda *size: torch.zeros(*size, dtype=torch.int32)
    torch.cuda.FloatTensor = lambda *size: torch.zeros(*size, dtype=torch.float32)
    p2 = "pcdet/ops/pointnet2/pointnet2_stack/"
    CR._load(f"{A}.ops.pointnet2.pointnet2_stack.pointnet2_utils", p2 + "pointnet2_utils.py")
    M["vq"] = CR._load(f"{A}.ops.pointnet2.pointnet2_stack.voxel_query_utils", p2 + "voxel_query_utils.py")
    M["vpm"] = CR._load(f"{A}.ops.pointnet2.pointnet2_stack.voxel_pool_modules", p2 + "voxel_pool_modules.py")
    M["head"] = CR._load(f"{A}.models.roi_heads.voxelrcnn_head", "pcdet/models/roi_heads/voxelrcnn_head.py")
    M["loss_utils"] = sys.modules[f"{A}.utils.loss_utils"]
    M["common_utils"] = sys.modules[f"{A}.utils.common_utils"]
    return M


class SparseLevel:
    """What the head reads of a spconv tensor: indices (b, z, y, x) int32, features, spatial_shape, batch_size."""

    def __init__(self, indices, features, spatial_shape, batch_size):
        self.indices, self.features, self.spatial_shape, self.batch_size = indices, features, spatial_shape, batch_size


def make_level(rng, batch, stride, occupancy):
    """Sites of a level at `stride`: every cell of the lattice with probability `occupancy`, rows in (b, z, y, x) order."""
    shape = [int(round((PC_RANGE[5] - PC_RANGE[2]) / VOXEL[2])) // stride, int(round((PC_RANGE[4] - PC_RANGE[1]) / VOXEL[1])) // stride,
             int(round((PC_RANGE[3] - PC_RANGE[0]) / VOXEL[0])) // stride]
    keep = rng.uniform(0, 1, [batch] + shape) < occupancy
    return np.argwhere(keep).astype(np.int32), shape


def cap_query(M):
    rng = np.random.default_rng(21)
    coords, shape = make_level(rng, 2, 2, 0.3)
    ct = torch.from_numpy(coords)
    xyz = M["common_utils"].get_voxel_centers(ct[:, 1:4], downsample_times=2, voxel_size=VOXEL, point_cloud_range=PC_RANGE)
    m_per = 300
    new_xyz = torch.from_numpy(rng.uniform([-25.0, -25.0, -3.5], [25.0, 25.0, 1.5], (2 * m_per, 3)).astype(np.float32))
    bidx = torch.arange(2).repeat_interleave(m_per).float().view(-1, 1)
    c = torch.cat([(new_xyz[:, j:j + 1] - PC_RANGE[j]) // VOXEL[j] for j in range(3)], 1) // 2
    new_coords = torch.cat([bidx, c], 1).int()[:, [0, 3, 2, 1]].contiguous()          # (b, z, y, x), as the pool module passes it
    level = SparseLevel(ct, None, shape, 2)
    v2p = M["common_utils"].generate_voxel2pinds(level)
    cnt = torch.tensor([(coords[:, 0] == b).sum() for b in range(2)], dtype=torch.int32)
    feats = torch.from_numpy(rng.standard_normal((len(coords), 3)).astype(np.float32))
    recorded = {}
    pu = sys.modules[f"{CR.ALIAS}.ops.pointnet2.pointnet2_stack.pointnet2_utils"]
    grouping = pu.grouping_operation

    def grouping_rec(features, features_batch_cnt, idx, idx_batch_cnt):
        recorded["idx"] = idx.numpy().copy()
        return grouping(features, features_batch_cnt, idx, idx_batch_cnt)

    M["vq"].pointnet2_utils.grouping_operation = grouping_rec
    rng_q = (2, 3, 3)
    TRACE["dist2_margin"] = np.inf
    grouper = M["vq"].VoxelQueryAndGrouping(rng_q, 0.9, 6)
    gf, gx, empty = grouper(new_coords, xyz, cnt, new_xyz, torch.tensor([m_per, m_per], dtype=torch.int32), feats, v2p)
    M["vq"].pointnet2_utils.grouping_operation = grouping
    assert TRACE["dist2_margin"] > 1e-5, TRACE["dist2_margin"]
    e = empty.numpy()
    assert e.any() and (~e).any()
    np.savez_compressed(os.path.join(OUT, "voxel_rcnn_query.npz"), coords=coords, shape=np.array(shape, np.int32), stride=np.int32(2),
                        new_xyz=new_xyz.numpy(), new_coords=new_coords.numpy(), radius=np.float64(0.9), query_range=np.array(rng_q, np.int32),
                        nsample=np.int32(6), idx=recorded["idx"], empty=e, grouped_features=gf.numpy())
    print("query: M", len(e), "empty", int(e.sum()), "dist2 margin", TRACE["dist2_margin"])


def pool_margin_ok(x):
    """x: the reference's ReLU output [1, C, M, nsample]: every positive maximum beats the next smaller value by > 1e-5 and
    lies > 1e-5 above 0 (equal values are the same voxel: the query's fill)."""
    v = x[0].detach()
    top = v.max(dim=-1, keepdim=True).values
    second = torch.where(v < top, v, torch.full_like(v, -1e30)).max(dim=-1).values
    top = top.squeeze(-1)
    pos = top > 0
    scale = torch.clamp(top.abs(), min=1.0)
    return bool(((top - second)[pos] > 1e-5 * scale[pos]).all()) and bool((top[pos] > 1e-5).all())


def head_inputs(rng, batch):
    levels, feats = {}, {}
    for name, stride, ch, _, _ in LEVELS:
        coords, shape = make_level(rng, batch, stride, 0.12 if stride == 2 else 0.4)
        f = rng.standard_normal((len(coords), ch)).astype(np.float32)
        levels[name] = (coords, shape, stride)
        feats[name] = f
    return levels, feats


def batch_dict(levels, feats, rois, scores, labels, grad=False):
    ms, st = {}, {}
    leaves = {}
    for name, (coords, shape, stride) in levels.items():
        f = torch.from_numpy(feats[name]).requires_grad_(grad)
        leaves[name] = f
        ms[name] = SparseLevel(torch.from_numpy(coords), f, shape, rois.shape[0])
        st[name] = stride
    return {"batch_size": rois.shape[0], "rois": torch.from_numpy(rois), "roi_scores": torch.from_numpy(scores),
            "roi_labels": torch.from_numpy(labels), "multi_scale_3d_features": ms, "multi_scale_3d_strides": st}, leaves


def cap_head(M):
    vpm = M["vpm"]
    real_f = vpm.F

    class RecordF:
        def __getattr__(self, k):
            return getattr(real_f, k)

        @staticmethod
        def max_pool2d(x, *a, **k):
            if TRACE["pool"] is not None:
                TRACE["pool"].append(pool_margin_ok(x))
            return real_f.max_pool2d(x, *a, **k)

    vpm.F = RecordF()
    rois, scores, labels, gt = CS.target_inputs(100)
    for attempt in range(60):
        rng = np.random.default_rng(500 + attempt)
        torch.manual_seed(3 + attempt)
        head = M["head"].VoxelRCNNHead(backbone_channels={n: c for n, _, c, _, _ in LEVELS}, model_cfg=head_cfg(),
                                       point_cloud_range=PC_RANGE, voxel_size=VOXEL, num_class=1)
        for m in head.modules():                  # non-trivial BN affine parameters and running statistics
            if isinstance(m, (torch.nn.BatchNorm1d, torch.nn.BatchNorm2d)):
                m.weight.data.uniform_(0.5, 1.5)
                m.bias.data.uniform_(-0.2, 0.2)
                m.running_mean.uniform_(-0.1, 0.1)
                m.running_var.uniform_(0.5, 1.5)
        state = {k: v.detach().numpy().copy() for k, v in head.state_dict().items()}
        levels, feats = head_inputs(rng, 3)
        TRACE["dist2_margin"] = np.inf
        head.eval()
        bd, _ = batch_dict(levels, feats, rois, scores, labels)
        with torch.no_grad():
            out = head(bd)
        eval_cls, eval_box = out["batch_cls_preds"].numpy(), out["batch_box_preds"].numpy()
        head.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()})
        head.train()
        bd, leaves = batch_dict(levels, feats, rois, scores, labels, grad=True)
        bd["gt_boxes"] = torch.from_numpy(gt)
        np.random.seed(9)
        torch.manual_seed(9)
        TRACE["pool"] = []
        head(bd)
        pool_ok = bool(TRACE["pool"]) and all(TRACE["pool"])
        TRACE["pool"] = None
        loss, tb = head.get_loss()
        loss.backward()
        with torch.no_grad():
            _, rec = CS.run_targets(M, rois, scores, labels, gt, 9)
        if TRACE["dist2_margin"] > 1e-5 and pool_ok and CS.margin_ok(np.stack(rec["max_iou"])):
            break
        print("attempt", attempt, "rejected: dist2 margin", TRACE["dist2_margin"], "pool margins", pool_ok)
    else:
        raise AssertionError("no seed keeps the radius, arg-max and sampler decisions off their thresholds")
    vpm.F = real_f
    grads = {f"grad.{k}": p.grad.numpy().copy() for k, p in head.named_parameters()}
    grads.update({f"fgrad.{n}": leaves[n].grad.numpy().copy() for n in leaves})
    fr = head.forward_ret_dict
    np.savez_compressed(
        os.path.join(OUT, "voxel_rcnn_head.npz"), rois=rois, roi_scores=scores, roi_labels=labels, gt_boxes=gt, seed=np.int64(9),
        pc_range=np.array(PC_RANGE, np.float64), voxel_size=np.array(VOXEL, np.float64), attempt=np.int64(attempt),
        keys=np.array(list(state.keys())), eval_cls=eval_cls, eval_box=eval_box,
        rcnn_loss=np.float32(loss.item()), **{f"tb.{k}": np.float32(v) for k, v in tb.items()},
        rcnn_cls_labels=fr["rcnn_cls_labels"].numpy(), reg_valid_mask=fr["reg_valid_mask"].numpy(), train_rois=fr["rois"].numpy(),
        **{f"coords.{n}": levels[n][0] for n in levels}, **{f"shape.{n}": np.array(levels[n][1], np.int32) for n in levels},
        **{f"stride.{n}": np.int32(levels[n][2]) for n in levels}, **{f"feat.{n}": feats[n] for n in feats},
        **{f"state.{k}": v for k, v in state.items()}, **grads)
    print("head: attempt", attempt, "keys", len(state), "loss", loss.item(), {k: float(v) for k, v in tb.items()})


def cap_corner(M):
    rng = np.random.default_rng(31)
    pred = rng.uniform([-5, -5, -1, 1, 1, 1, -3], [5, 5, 1, 4, 3, 2, 3], (24, 7)).astype(np.float32)
    gt = (pred + rng.normal(0, 0.4, (24, 7))).astype(np.float32)
    gt[:6, 6] += np.pi                                          # heading-flipped gts
    out = M["loss_utils"].get_corner_loss_lidar(torch.from_numpy(pred), torch.from_numpy(gt))
    np.savez_compressed(os.path.join(OUT, "voxel_rcnn_corner.npz"), pred=pred, gt=gt, loss=out.numpy())
    print("corner", out.shape)


def main():
    M = setup()
    cap_query(M)
    cap_head(M)
    cap_corner(M)


if __name__ == "__main__":
    main()
