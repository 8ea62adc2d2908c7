"""Rotated BEV overlap of the KITTI evaluator (reference kitti_object_eval_python/rotate_iou.py, a numba-CUDA kernel) on
toda_eval_overlaps: exact clipping without a corner margin, angles clockwise-positive."""
import numpy as np


def rotate_iou_gpu_eval(boxes, query_boxes, criterion=-1, device_id=0):
    """boxes [N, 5], query_boxes [K, 5] = (cx, cy, dx, dy, angle), numpy in -> [N, K] numpy out in boxes' dtype.
    criterion -1: IoU; 0: intersection / query area; 1: / box area (the kernel takes the query first); 2: the intersection."""
    import torch

    from ..... import ops
    boxes, query_boxes = np.asarray(boxes), np.asarray(query_boxes)
    n, k = boxes.shape[0], query_boxes.shape[0]
    if n == 0 or k == 0:
        return np.zeros((n, k), dtype=np.float32).astype(boxes.dtype)
    if not torch.cuda.is_available():
        raise RuntimeError("rotate_iou_gpu_eval needs a GPU (there is no CPU path)")
    dev = torch.device("cuda", device_id)

    def rows(b):        # (cx, cy, dx, dy, angle) -> x, y, z, l, h, w, ry with the rectangle in the x-z plane
        r = np.zeros((len(b), 7), np.float32)
        r[:, [0, 2, 3, 5, 6]] = b[:, :5].astype(np.float32)
        return torch.from_numpy(r).to(dev)

    with torch.cuda.device(dev):
        out = ops.eval_overlaps(rows(boxes), None, torch.tensor([0, n], dtype=torch.int32, device=dev), rows(query_boxes), None,
                                torch.tensor([0, k], dtype=torch.int32, device=dev),
                                torch.tensor([0, n * k], dtype=torch.int64, device=dev), n * k, 1, criterion)
        return out.reshape(n, k).cpu().numpy().astype(boxes.dtype)
