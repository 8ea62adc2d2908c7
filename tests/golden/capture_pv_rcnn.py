#!/usr/bin/env python
"""Capture golden vectors from the REFERENCE's PV-RCNN modules (build container only, CPU).

    python tests/golden/capture_pv_rcnn.py
writes tests/golden/pv_rcnn_ops.npz (FPS index sequences on clouds with exact ties and duplicated points, N on both sides of
1024 and one N < npoint; a stacked ball-query table), pv_rcnn_vsa.npz (a small VoxelSetAbstraction: state dict, inputs,
point_coords / point_features_before_fusion / point_features in training mode), pv_rcnn_point_head.npz (PointHeadSimple: state,
inputs, point_cls_scores, stack targets, focal loss) and pv_rcnn_head.npz (a small PVRCNNHead: state dict, eval-mode
batch_cls_preds / batch_box_preds, train-mode loss terms and gradients with DP_RATIO 0).

pcdet/models/backbones_3d/pfe/voxel_set_abstraction.py, dense_heads/point_head_{template,simple}.py, roi_heads/pvrcnn_head.py and
ops/pointnet2/pointnet2_stack/{pointnet2_utils,pointnet2_modules}.py are loaded by path (capture_voxel_rcnn.setup()).  Their
compiled helpers cannot be built in this image, so farthest_point_sampling_wrapper, ball_query_wrapper (pointnet2_stack_cuda) and
points_in_boxes_gpu (roiaware_pool3d_cuda) are served by numpy stand-ins written from src/sampling_gpu.cu (T threads of stride
T, the first maximum per thread, the block's halving tree), src/ball_query_gpu.cu and roiaware_pool3d_kernel.cu.  No candidate's
d2 lies within 1e-5 (relative) of radius^2, no point lies within 1e-4 of a box face, and in training no pooled maximum lies
within 1e-5 of another value or of 0 (all asserted below), so last-bit differences of a device evaluation cannot flip a neighbour,
a label or an arg-max.  The roi sampler's IoUs come from the oracle as in capture_second_head.py, with its margin check.
Only inputs, parameters, seeds and outputs are stored - no reference source.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import capture_reference as CR  # noqa: E402
import capture_second_head as CS  # noqa: E402
import capture_voxel_rcnn as CV  # noqa: E402
from capture_reference import EasyDict  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
PC_RANGE = [-24.0, -24.0, -3.0, 24.0, 24.0, 1.0]
VOXEL = [0.4, 0.4, 0.5]
TRACE = {"d2": np.inf, "box": np.inf, "pool": None}


def opt_n_threads(n):
    import math
    return max(min(1 << int(math.log(float(n)) / math.log(2.0)), 1024), 1)


def farthest_point_sampling_wrapper(b, n, m, points, temp, idxs):
    """sampling_gpu.cu:25-140 in numpy fp32: thread t takes k = t, t + T, ... and keeps its first maximum (strict >), then the
    halving tree keeps the lower slot on a tie."""
    xyz = points.numpy().reshape(b, n, 3)
    out = idxs.numpy().reshape(b, m)
    t = opt_n_threads(n)
    rows = -(-n // t)
    for s in range(b):
        x = xyz[s]
        tmp = temp.numpy().reshape(b, n)[s].copy()
        old = 0
        out[s, 0] = 0
        for j in range(1, m):
            diff = x - x[old]
            d = np.float32(diff[:, 0] * diff[:, 0] + diff[:, 1] * diff[:, 1]) + diff[:, 2] * diff[:, 2]
            tmp = np.minimum(d.astype(np.float32), tmp)
            pad = np.full((rows * t,), -1.0, np.float32)
            pad[:n] = tmp
            grid = pad.reshape(rows, t)
            arg = grid.argmax(0)                                    # first maximum of each thread
            dists = grid[arg, np.arange(t)]
            di = arg * t + np.arange(t)
            w = t
            while w > 1:
                w //= 2
                v1, v2 = dists[:w].copy(), dists[w:2 * w]
                i1, i2 = di[:w].copy(), di[w:2 * w]
                dists[:w] = np.maximum(v1, v2)
                di[:w] = np.where(v2 > v1, i2, i1)
            old = int(di[0])
            out[s, j] = old


def ball_query_wrapper(B, M, radius, nsample, new_xyz, new_xyz_batch_cnt, xyz, xyz_batch_cnt, idx):
    """ball_query_gpu.cu:15-64 in numpy fp32; records how close any d2 comes to radius^2."""
    nx, px, out = new_xyz.numpy(), xyz.numpy(), idx.numpy()
    ncnt, pcnt = new_xyz_batch_cnt.numpy(), xyz_batch_cnt.numpy()
    r2 = np.float32(radius) * np.float32(radius)
    q0 = np.concatenate([[0], np.cumsum(ncnt)])
    p0 = np.concatenate([[0], np.cumsum(pcnt)])
    for b in range(B):
        pts = px[p0[b]:p0[b + 1]]
        for m in range(q0[b], q0[b + 1]):
            c = nx[m]
            d2 = np.float32(np.float32((c[0] - pts[:, 0]) * (c[0] - pts[:, 0])) + np.float32((c[1] - pts[:, 1]) * (c[1] - pts[:, 1]))) \
                + np.float32((c[2] - pts[:, 2]) * (c[2] - pts[:, 2]))
            d2 = d2.astype(np.float32)
            if len(d2):
                TRACE["d2"] = min(TRACE["d2"], float(np.min(np.abs(d2 - r2))) / float(r2))
            hits = np.nonzero(d2 < r2)[0][:nsample]
            if len(hits) == 0:
                out[m, 0] = -1
                continue
            out[m, :] = hits[0]
            out[m, :len(hits)] = hits


def points_in_boxes_gpu(boxes, pts, box_idx_of_points):
    """roiaware_pool3d_kernel.cu points_in_boxes_kernel: the first box whose test passes (|z - cz| <= dz / 2, |local| < d / 2 +
    1e-5 after rotating by -heading); records how close a point comes to a face of a non-empty box."""
    bx, p, out = boxes.numpy(), pts.numpy(), box_idx_of_points.numpy()
    for b in range(bx.shape[0]):
        for k in range(bx.shape[1]):
            cx, cy, cz, dx, dy, dz, rz = (np.float32(v) for v in bx[b, k])
            cosa, sina = np.float32(np.cos(-rz)), np.float32(np.sin(-rz))
            sx, sy = p[b, :, 0] - cx, p[b, :, 1] - cy
            lx = sx * cosa + sy * (-sina)
            ly = sx * sina + sy * cosa
            zin = np.abs(p[b, :, 2] - cz) <= dz / 2.0
            inside = zin & (np.abs(lx) < dx / 2.0 + 1e-5) & (np.abs(ly) < dy / 2.0 + 1e-5)
            if dx > 0:
                gap = np.minimum(np.minimum(np.abs(np.abs(lx) - dx / 2.0), np.abs(np.abs(ly) - dy / 2.0)), np.abs(np.abs(p[b, :, 2] - cz) - dz / 2.0))
                TRACE["box"] = min(TRACE["box"], float(gap.min()))
            free = out[b] < 0
            out[b][free & inside] = k
    return out


def setup():
    M = CV.setup()
    A = CR.ALIAS
    cu = sys.modules[f"{A}.ops.pointnet2.pointnet2_stack.pointnet2_stack_cuda"]
    cu.farthest_point_sampling_wrapper = farthest_point_sampling_wrapper
    cu.ball_query_wrapper = ball_query_wrapper
    sys.modules[f"{A}.ops.roiaware_pool3d.roiaware_pool3d_cuda"].points_in_boxes_gpu = points_in_boxes_gpu
    for name in (f"{A}.models.backbones_3d.pfe",):
        CR._pkg(name)
    p2 = "pcdet/ops/pointnet2/pointnet2_stack/"
    M["pu"] = sys.modules[f"{A}.ops.pointnet2.pointnet2_stack.pointnet2_utils"]
    M["pm"] = CR._load(f"{A}.ops.pointnet2.pointnet2_stack.pointnet2_modules", p2 + "pointnet2_modules.py")
    M["vsa"] = CR._load(f"{A}.models.backbones_3d.pfe.voxel_set_abstraction", "pcdet/models/backbones_3d/pfe/voxel_set_abstraction.py")
    CR._load(f"{A}.models.dense_heads.point_head_template", "pcdet/models/dense_heads/point_head_template.py")
    M["phs"] = CR._load(f"{A}.models.dense_heads.point_head_simple", "pcdet/models/dense_heads/point_head_simple.py")
    M["pvh"] = CR._load(f"{A}.models.roi_heads.pvrcnn_head", "pcdet/models/roi_heads/pvrcnn_head.py")
    return M


def lattice(rng, n, lo, hi, step):
    return (np.round(rng.uniform(lo, hi, (n, 3)) / step) * step).astype(np.float32)


def cap_ops(M):
    rng = np.random.default_rng(7)
    out = {}
    for tag, n, npoint in (("a", 700, 256), ("b", 1500, 400), ("c", 90, 128)):
        x = lattice(rng, n, [-6, -6, -1], [6, 6, 1], 0.25)          # coarse lattice: exact ties
        x[-40:] = x[:40]                                             # duplicated points
        idx = M["pu"].farthest_point_sample(torch.from_numpy(x).unsqueeze(0).contiguous(), npoint)
        out[f"fps_{tag}_xyz"], out[f"fps_{tag}_idx"] = x, idx.numpy()[0]
    xyz = rng.uniform([-5, -5, -1], [5, 5, 1], (500, 3)).astype(np.float32)
    new_xyz = rng.uniform([-5.5, -5.5, -1.2], [5.5, 5.5, 1.2], (80, 3)).astype(np.float32)
    TRACE["d2"] = np.inf
    idx, empty = M["pu"].ball_query(0.7, 12, torch.from_numpy(xyz), torch.tensor([300, 200], dtype=torch.int32), torch.from_numpy(new_xyz),
                                    torch.tensor([50, 30], dtype=torch.int32))
    assert TRACE["d2"] > 1e-5, TRACE["d2"]
    assert empty.any() and (~empty).any()
    np.savez_compressed(os.path.join(OUT, "pv_rcnn_ops.npz"), bq_xyz=xyz, bq_new_xyz=new_xyz, bq_idx=idx.numpy(), bq_empty=empty.numpy(),
                        bq_counts=np.array([300, 200], np.int32), bq_new_counts=np.array([50, 30], np.int32), bq_radius=np.float64(0.7),
                        bq_nsample=np.int32(12), **out)
    print("ops: d2 margin", TRACE["d2"], "empty", int(empty.sum()))


def vsa_cfg():
    return EasyDict(dict(
        NAME="VoxelSetAbstraction", POINT_SOURCE="raw_points", NUM_KEYPOINTS=48, NUM_OUTPUT_FEATURES=16, SAMPLE_METHOD="FPS",
        FEATURES_SOURCE=["bev", "x_conv3", "raw_points"],
        SA_LAYER=dict(raw_points=dict(MLPS=[[8, 8], [8, 8]], POOL_RADIUS=[0.8, 1.6], NSAMPLE=[8, 16]),
                      x_conv3=dict(DOWNSAMPLE_FACTOR=4, MLPS=[[6, 8], [6, 8]], POOL_RADIUS=[1.6, 3.2], NSAMPLE=[8, 16]))))


def randomise_bn(module):
    for m in module.modules():
        if isinstance(m, (torch.nn.BatchNorm1d, torch.nn.BatchNorm2d)):
            m.weight.data.uniform_(0.5, 1.5)
            m.bias.data.uniform_(-0.2, 0.2)
            m.running_mean.uniform_(-0.1, 0.1)
            m.running_var.uniform_(0.5, 1.5)


def cap_vsa(M):
    for attempt in range(40):
        rng = np.random.default_rng(100 + attempt)
        torch.manual_seed(100 + attempt)
        pts = []
        for b in range(2):
            p = rng.uniform([-20, -20, -2.5, 0], [20, 20, 0.5, 1], (400, 4)).astype(np.float32)
            pts.append(np.concatenate([np.full((400, 1), b, np.float32), p], 1))
        points = np.concatenate(pts, 0)
        coords, shape = CV.make_level(rng, 2, 4, 0.5)
        feats = rng.standard_normal((len(coords), 6)).astype(np.float32)
        bev = rng.standard_normal((2, 10, 15, 15)).astype(np.float32)
        vsa = M["vsa"].VoxelSetAbstraction(vsa_cfg(), voxel_size=VOXEL, point_cloud_range=PC_RANGE, num_bev_features=10, num_rawpoint_features=4)
        randomise_bn(vsa)
        for p in vsa.parameters():
            p.data.add_(torch.randn_like(p) * 0.05)
        state = {k: v.detach().numpy().copy() for k, v in vsa.state_dict().items()}
        vsa.train()
        TRACE["d2"] = np.inf
        bd = {"batch_size": 2, "points": torch.from_numpy(points), "spatial_features": torch.from_numpy(bev), "spatial_features_stride": 8,
              "multi_scale_3d_features": {"x_conv3": CV.SparseLevel(torch.from_numpy(coords), torch.from_numpy(feats), shape, 2)}}
        with torch.no_grad():
            bd = vsa(bd)
        if TRACE["d2"] > 1e-5:
            break
        print("vsa attempt", attempt, "rejected: d2 margin", TRACE["d2"])
    else:
        raise AssertionError("no seed keeps the radius decisions off their threshold")
    np.savez_compressed(os.path.join(OUT, "pv_rcnn_vsa.npz"), points=points, coords=coords, shape=np.array(shape, np.int32), feats=feats, bev=bev,
                        keys=np.array(list(state.keys())), **{f"state.{k}": v for k, v in state.items()},
                        point_coords=bd["point_coords"].numpy(), before_fusion=bd["point_features_before_fusion"].numpy(),
                        point_features=bd["point_features"].numpy(), **{f"running.{k}": v.numpy() for k, v in vsa.state_dict().items()})
    print("vsa: attempt", attempt, "d2 margin", TRACE["d2"], "features", bd["point_features"].shape)


def point_head_cfg():
    return EasyDict(dict(NAME="PointHeadSimple", CLS_FC=[16, 16], CLASS_AGNOSTIC=True, USE_POINT_FEATURES_BEFORE_FUSION=True,
                         TARGET_CONFIG=dict(GT_EXTRA_WIDTH=[0.2, 0.2, 0.2]),
                         LOSS_CONFIG=dict(LOSS_REG="smooth-l1", LOSS_WEIGHTS={"point_cls_weight": 1.0})))


def cap_point_head(M):
    rois, scores, labels, gt = CS.target_inputs(100)
    for attempt in range(40):
        rng = np.random.default_rng(300 + attempt)
        torch.manual_seed(300 + attempt)
        coords = []
        for b in range(3):
            src = gt[b, :, :3] if gt[b, :, 3].any() else rois[b, :6, :3]
            near = src[rng.integers(0, len(src), 60)] + rng.normal(0, [1.5, 1.5, 0.6], (60, 3))
            coords.append(np.concatenate([np.full((100, 1), b), np.concatenate([near, rng.uniform(-20, 20, (40, 3))], 0)], 1))
        coords = np.concatenate(coords, 0).astype(np.float32)
        feats = rng.standard_normal((300, 12)).astype(np.float32)
        head = M["phs"].PointHeadSimple(num_class=1, input_channels=12, model_cfg=point_head_cfg())
        randomise_bn(head)
        state = {k: v.detach().numpy().copy() for k, v in head.state_dict().items()}
        head.train()
        TRACE["box"] = np.inf
        bd = {"batch_size": 3, "point_coords": torch.from_numpy(coords), "point_features_before_fusion": torch.from_numpy(feats),
              "gt_boxes": torch.from_numpy(gt)}
        bd = head(bd)
        labels_pt = head.forward_ret_dict["point_cls_labels"].numpy()
        if TRACE["box"] > 1e-4 and (labels_pt == 1).any() and (labels_pt == -1).any():
            break
        print("point head attempt", attempt, "rejected: box margin", TRACE["box"])
    else:
        raise AssertionError("no seed keeps the points off the box faces")
    loss, tb = head.get_loss()
    np.savez_compressed(os.path.join(OUT, "pv_rcnn_point_head.npz"), coords=coords, feats=feats, gt_boxes=gt,
                        keys=np.array(list(state.keys())), **{f"state.{k}": v for k, v in state.items()},
                        point_cls_scores=bd["point_cls_scores"].detach().numpy(), point_cls_preds=head.forward_ret_dict["point_cls_preds"].detach().numpy(),
                        point_cls_labels=labels_pt, loss=np.float32(loss.item()), pos_num=np.float32(tb["point_pos_num"]))
    print("point head: attempt", attempt, "box margin", TRACE["box"], "labels", np.unique(labels_pt, return_counts=True), "loss", loss.item())


def pv_head_cfg():
    return EasyDict(dict(
        NAME="PVRCNNHead", CLASS_AGNOSTIC=True, SHARED_FC=[16, 16], CLS_FC=[16, 16], REG_FC=[16, 16], DP_RATIO=0.0,
        NMS_CONFIG=dict(TRAIN=dict(NMS_TYPE="nms_gpu", MULTI_CLASSES_NMS=False, NMS_PRE_MAXSIZE=9000, NMS_POST_MAXSIZE=512, NMS_THRESH=0.8),
                        TEST=dict(NMS_TYPE="nms_gpu", MULTI_CLASSES_NMS=False, NMS_PRE_MAXSIZE=1024, NMS_POST_MAXSIZE=100, NMS_THRESH=0.7)),
        ROI_GRID_POOL=dict(GRID_SIZE=3, MLPS=[[8, 8], [8, 8]], POOL_RADIUS=[0.8, 1.6], NSAMPLE=[8, 8], POOL_METHOD="max_pool"),
        TARGET_CONFIG=CS.TARGET_CONFIG,
        LOSS_CONFIG=dict(CLS_LOSS="BinaryCrossEntropy", REG_LOSS="smooth-l1", CORNER_LOSS_REGULARIZATION=True,
                         LOSS_WEIGHTS=dict(rcnn_cls_weight=1.0, rcnn_reg_weight=1.0, rcnn_corner_weight=1.0, code_weights=[1.0] * 7))))


def head_points(rng, rois):
    """240 keypoints per sample: 200 around the rois' centres, 40 uniform; features and scores."""
    coords = []
    for b in range(rois.shape[0]):
        near = rois[b, rng.integers(0, rois.shape[1], 200), :3] + rng.normal(0, [1.2, 1.2, 0.5], (200, 3))
        coords.append(np.concatenate([np.full((240, 1), b), np.concatenate([near, rng.uniform(-20, 20, (40, 3))], 0)], 1))
    coords = np.concatenate(coords, 0).astype(np.float32)
    return coords, rng.standard_normal((len(coords), 6)).astype(np.float32), rng.uniform(0.05, 0.95, len(coords)).astype(np.float32)


def cap_head(M):
    pm = M["pm"]
    real_f = pm.F

    class RecordF:
        def __getattr__(self, k):
            return getattr(real_f, k)

        @staticmethod
        def max_pool2d(x, *a, **k):
            if TRACE["pool"] is not None:
                TRACE["pool"].append(CV.pool_margin_ok(x))
            return real_f.max_pool2d(x, *a, **k)

    pm.F = RecordF()
    rois, scores, labels, gt = CS.target_inputs(100)
    for attempt in range(60):
        rng = np.random.default_rng(700 + attempt)
        torch.manual_seed(7 + attempt)
        head = M["pvh"].PVRCNNHead(input_channels=6, model_cfg=pv_head_cfg(), num_class=1)
        randomise_bn(head)
        state = {k: v.detach().numpy().copy() for k, v in head.state_dict().items()}
        coords, feats, pscores = head_points(rng, rois)

        def bd(grad=False):
            f = torch.from_numpy(feats).requires_grad_(grad)
            return {"batch_size": 3, "rois": torch.from_numpy(rois), "roi_scores": torch.from_numpy(scores), "roi_labels": torch.from_numpy(labels),
                    "point_coords": torch.from_numpy(coords), "point_features": f, "point_cls_scores": torch.from_numpy(pscores)}, f

        TRACE["d2"] = np.inf
        head.eval()
        with torch.no_grad():
            out = head(bd()[0])
        eval_cls, eval_box = out["batch_cls_preds"].numpy(), out["batch_box_preds"].numpy()
        head.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()})
        head.train()
        d, leaf = bd(grad=True)
        d["gt_boxes"] = torch.from_numpy(gt)
        np.random.seed(9)
        torch.manual_seed(9)
        TRACE["pool"] = []
        head(d)
        pool_ok = bool(TRACE["pool"]) and all(TRACE["pool"])
        TRACE["pool"] = None
        loss, tb = head.get_loss()
        loss.backward()
        with torch.no_grad():
            _, rec = CS.run_targets(M, rois, scores, labels, gt, 9)
        if TRACE["d2"] > 1e-5 and pool_ok and CS.margin_ok(np.stack(rec["max_iou"])):
            break
        print("head attempt", attempt, "rejected: d2 margin", TRACE["d2"], "pool margins", pool_ok)
    else:
        raise AssertionError("no seed keeps the radius, arg-max and sampler decisions off their thresholds")
    pm.F = real_f
    grads = {f"grad.{k}": p.grad.numpy().copy() for k, p in head.named_parameters()}
    fr = head.forward_ret_dict
    np.savez_compressed(
        os.path.join(OUT, "pv_rcnn_head.npz"), rois=rois, roi_scores=scores, roi_labels=labels, gt_boxes=gt, seed=np.int64(9),
        point_coords=coords, point_features=feats, point_cls_scores=pscores, attempt=np.int64(attempt),
        keys=np.array(list(state.keys())), eval_cls=eval_cls, eval_box=eval_box, fgrad=leaf.grad.numpy().copy(),
        rcnn_loss=np.float32(loss.item()), **{f"tb.{k}": np.float32(v) for k, v in tb.items()},
        rcnn_cls_labels=fr["rcnn_cls_labels"].numpy(), reg_valid_mask=fr["reg_valid_mask"].numpy(), train_rois=fr["rois"].numpy(),
        **{f"state.{k}": v for k, v in state.items()}, **grads)
    print("head: attempt", attempt, "keys", len(state), "loss", loss.item(), {k: float(v) for k, v in tb.items()})


def main():
    M = setup()
    cap_ops(M)
    cap_vsa(M)
    cap_point_head(M)
    cap_head(M)


if __name__ == "__main__":
    main()
