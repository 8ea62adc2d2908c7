"""Box helpers on the anchor-head path and the KITTI camera-frame conversions (reference pcdet/utils/box_utils.py)."""
import numpy as np
import torch

from . import common_utils


def boxes_iou_normal(boxes_a, boxes_b):
    """Axis-aligned IoU of [N,4] x [M,4] boxes (x1, y1, x2, y2)."""
    assert boxes_a.shape[1] == boxes_b.shape[1] == 4
    lo = torch.max(boxes_a[:, None, 0:2], boxes_b[None, :, 0:2])
    hi = torch.min(boxes_a[:, None, 2:4], boxes_b[None, :, 2:4])
    wh = torch.clamp_min(hi - lo, min=0)
    inter = wh[..., 0] * wh[..., 1]
    area_a = (boxes_a[:, 2] - boxes_a[:, 0]) * (boxes_a[:, 3] - boxes_a[:, 1])
    area_b = (boxes_b[:, 2] - boxes_b[:, 0]) * (boxes_b[:, 3] - boxes_b[:, 1])
    return inter / torch.clamp_min(area_a[:, None] + area_b[None, :] - inter, min=1e-6)


def boxes3d_lidar_to_aligned_bev_boxes(boxes3d):
    """Snap headings to the nearest axis: boxes whose |heading mod pi| >= pi/4 swap dx and dy."""
    rot = common_utils.limit_period(boxes3d[:, 6], offset=0.5, period=np.pi).abs()
    dims = torch.where(rot[:, None] < np.pi / 4, boxes3d[:, [3, 4]], boxes3d[:, [4, 3]])
    return torch.cat((boxes3d[:, 0:2] - dims / 2, boxes3d[:, 0:2] + dims / 2), dim=1)


def boxes3d_nearest_bev_iou(boxes_a, boxes_b):
    return boxes_iou_normal(boxes3d_lidar_to_aligned_bev_boxes(boxes_a), boxes3d_lidar_to_aligned_bev_boxes(boxes_b))


_CORNER_SIGNS = ((1, 1, -1), (1, -1, -1), (-1, -1, -1), (-1, 1, -1), (1, 1, 1), (1, -1, 1), (-1, -1, 1), (-1, 1, 1))


def boxes_to_corners_3d(boxes3d):
    """[N, >=7] (x y z dx dy dz heading) -> [N, 8, 3]; corners 0-3 bottom (+x+y, +x-y, -x-y, -x+y), 4-7 top, same
    order as the reference (box_utils.py:28-54).  fp32 torch arithmetic, numpy in -> numpy out."""
    boxes3d, is_numpy = common_utils.check_numpy_to_torch(boxes3d)
    half = boxes3d.new_tensor(_CORNER_SIGNS) / 2
    local = boxes3d[:, None, 3:6].repeat(1, 8, 1) * half[None, :, :]
    corners = common_utils.rotate_points_along_z(local.view(-1, 8, 3), boxes3d[:, 6]).view(-1, 8, 3)
    corners += boxes3d[:, None, 0:3]
    return corners.numpy() if is_numpy else corners


def mask_boxes_outside_range_numpy(boxes, limit_range, min_num_corners=1):
    """True for boxes with at least `min_num_corners` of their 8 corners inside [min xyz, max xyz], ends inclusive
    (reference box_utils.py:57-72; all three coordinates are tested)."""
    if boxes.shape[0] == 0:
        return np.zeros((0,), dtype=bool)
    corners = boxes_to_corners_3d(boxes[:, 0:7])
    lim = np.asarray(limit_range)
    inside = ((corners >= lim[0:3]) & (corners <= lim[3:6])).all(axis=2)
    return inside.sum(axis=1) >= min_num_corners


def enlarge_box3d(boxes3d, extra_width=(0, 0, 0)):
    """dx, dy, dz grown by extra_width (reference box_utils.py:145-158); returns a torch tensor like the reference."""
    boxes3d, _ = common_utils.check_numpy_to_torch(boxes3d)
    large = boxes3d.clone()
    large[:, 3:6] += boxes3d.new_tensor(extra_width)[None, :]
    return large


def remove_points_in_boxes3d(points, boxes3d):
    """points [N, 3+C] without those inside any of boxes3d [M, 7] (reference box_utils.py:75-89).  CUDA clouds are filtered
    by the in-box kernel + a stable compaction and stay on the device; numpy / CPU clouds take the same route and come back."""
    from toda_amd import ops

    is_numpy = isinstance(points, np.ndarray)
    was_cuda = torch.is_tensor(points) and points.is_cuda
    pts = torch.as_tensor(points, dtype=torch.float32).cuda().contiguous()
    bx = torch.as_tensor(np.asarray(boxes3d.cpu() if torch.is_tensor(boxes3d) else boxes3d), dtype=torch.float32)[:, :7].cuda().contiguous()
    if bx.shape[0] and pts.shape[0]:
        flags = ops.points_in_boxes(pts, bx, mode=0)
        pts = ops.RowBuffer(pts.shape[0], pts.shape[1], pts.device).append(pts, flags, 1, invert=True).finish()
    if was_cuda:
        return pts
    return pts.cpu().numpy() if is_numpy else pts.cpu()


# ---- KITTI camera-frame boxes (reference box_utils.py:92-108, 161-246).  At most a few hundred boxes per frame, and the results
# are host annotation dicts: numpy, no kernel.
def boxes3d_kitti_camera_to_lidar(boxes3d_camera, calib):
    """[N, 7] (x y z l h w ry; rectified camera frame, y at the bottom face) -> (x y z dx dy dz heading), z at the box centre."""
    cam = np.array(boxes3d_camera, copy=True)
    xyz = calib.rect_to_lidar(cam[:, 0:3])
    xyz[:, 2] += cam[:, 4] / 2
    return np.concatenate([xyz, cam[:, 3:4], cam[:, 5:6], cam[:, 4:5], -(cam[:, 6:7] + np.pi / 2)], axis=-1)


def boxes3d_kitti_fakelidar_to_lidar(boxes3d_fakelidar):
    """[N, 7+] (x y z w l h r; the older LiDAR layout, z at the bottom face) -> (x y z dx dy dz heading), z at the box centre
    (reference box_utils.py:111-125); columns past the seventh are dropped, as there."""
    old = np.array(boxes3d_fakelidar, copy=True)
    old[:, 2] += old[:, 5] / 2
    return np.concatenate([old[:, 0:3], old[:, 4:5], old[:, 3:4], old[:, 5:6], -(old[:, 6:7] + np.pi / 2)], axis=-1)


def boxes3d_lidar_to_kitti_camera(boxes3d_lidar, calib):
    """The inverse map: [N, 7] LiDAR boxes -> (x y z l h w ry) in the rectified camera frame."""
    lidar = np.array(boxes3d_lidar, copy=True)
    xyz = lidar[:, 0:3]
    xyz[:, 2] -= lidar[:, 5] / 2
    return np.concatenate([calib.lidar_to_rect(xyz), lidar[:, 3:4], lidar[:, 5:6], lidar[:, 4:5], -lidar[:, 6:7] - np.pi / 2], axis=-1)


def boxes3d_to_corners3d_kitti_camera(boxes3d, bottom_center=True):
    """[N, 7] camera boxes -> fp32 corners [N, 8, 3]: 0-3 the bottom face (+l+w, +l-w, -l-w, -l+w), 4-7 above them (-y is up);
    bottom_center: y is the bottom face's height, else the centre's."""
    n = boxes3d.shape[0]
    half_l, half_w = boxes3d[:, 3:4] / 2.0, boxes3d[:, 5:6] / 2.0
    h = boxes3d[:, 4:5]
    sx = np.array([1, 1, -1, -1, 1, 1, -1, -1], dtype=np.float32)
    sz = np.array([1, -1, -1, 1, 1, -1, -1, 1], dtype=np.float32)
    x_local = (half_l * sx).astype(np.float32)
    z_local = (half_w * sz).astype(np.float32)
    if bottom_center:
        y_local = np.zeros((n, 8), dtype=np.float32)
        y_local[:, 4:8] = -h
    else:
        y_local = (h / 2.0 * np.array([1, 1, 1, 1, -1, -1, -1, -1], dtype=np.float32)).astype(np.float32)
    ry = boxes3d[:, 6]
    zeros, ones = np.zeros(ry.size, dtype=np.float32), np.ones(ry.size, dtype=np.float32)
    rot = np.transpose(np.array([[np.cos(ry), zeros, -np.sin(ry)], [zeros, ones, zeros], [np.sin(ry), zeros, np.cos(ry)]]), (2, 0, 1))
    turned = np.matmul(np.stack([x_local, y_local, z_local], axis=2), rot)
    return (turned + boxes3d[:, None, 0:3]).astype(np.float32)


def boxes3d_kitti_camera_to_imageboxes(boxes3d, calib, image_shape=None):
    """[N, 7] camera boxes -> [N, 4] (x1 y1 x2 y2): the pixel extent of the eight corners, clipped to the image
    ([0, width - 1] x [0, height - 1]) when image_shape = (height, width) is given."""
    corners = boxes3d_to_corners3d_kitti_camera(boxes3d)
    pixels, _ = calib.rect_to_img(corners.reshape(-1, 3))
    pixels = pixels.reshape(-1, 8, 2)
    boxes2d = np.concatenate([pixels.min(axis=1), pixels.max(axis=1)], axis=1)
    if image_shape is not None:
        boxes2d[:, 0::2] = np.clip(boxes2d[:, 0::2], a_min=0, a_max=image_shape[1] - 1)
        boxes2d[:, 1::2] = np.clip(boxes2d[:, 1::2], a_min=0, a_max=image_shape[0] - 1)
    return boxes2d
