"""Global, per-object and pyramid augmentations (reference pcdet/datasets/augmentor/augmentor_utils.py), same names, same
random draws.  numpy clouds are transformed on the host with the reference's expressions; CUDA clouds by fused kernels
(toda_points_world_transform, toda_points_box_steps, toda_points_in_pyramids).  The boxes (a few dozen rows) are always
handled on the host."""
import numpy as np
import torch

from ...utils import common_utils


def _on_device(points):
    return torch.is_tensor(points) and points.is_cuda


def random_flip_along_x(gt_boxes, points, return_flip=False):
    enable = np.random.choice([False, True], replace=False, p=[0.5, 0.5])
    if enable:
        gt_boxes[:, 1] = -gt_boxes[:, 1]
        gt_boxes[:, 6] = -gt_boxes[:, 6]
        if _on_device(points):
            from .... import ops
            points = ops.points_world_transform(points.contiguous(), flip_x=True)
        else:
            points[:, 1] = -points[:, 1]
        if gt_boxes.shape[1] > 8:
            gt_boxes[:, 8] = -gt_boxes[:, 8]
    return (gt_boxes, points, enable) if return_flip else (gt_boxes, points)


def random_flip_along_y(gt_boxes, points, return_flip=False):
    enable = np.random.choice([False, True], replace=False, p=[0.5, 0.5])
    if enable:
        gt_boxes[:, 0] = -gt_boxes[:, 0]
        gt_boxes[:, 6] = -(gt_boxes[:, 6] + np.pi)
        if _on_device(points):
            from .... import ops
            points = ops.points_world_transform(points.contiguous(), flip_y=True)
        else:
            points[:, 0] = -points[:, 0]
        if gt_boxes.shape[1] > 8:
            gt_boxes[:, 7] = -gt_boxes[:, 7]
    return (gt_boxes, points, enable) if return_flip else (gt_boxes, points)


def global_rotation(gt_boxes, points, rot_range, return_rot=False):
    noise_rotation = np.random.uniform(rot_range[0], rot_range[1])
    angle = np.array([noise_rotation])
    if _on_device(points):
        from .... import ops
        a = torch.from_numpy(angle).float()                       # the reference rotates with fp32 cos / sin of the fp32 angle
        points = ops.points_world_transform(points.contiguous(), rot=(float(torch.cos(a)), float(torch.sin(a))))
    else:
        points = common_utils.rotate_points_along_z(points[np.newaxis, :, :], angle)[0]
    gt_boxes[:, 0:3] = common_utils.rotate_points_along_z(gt_boxes[np.newaxis, :, 0:3], angle)[0]
    gt_boxes[:, 6] += noise_rotation
    if gt_boxes.shape[1] > 8:
        vel = np.hstack((gt_boxes[:, 7:9], np.zeros((gt_boxes.shape[0], 1))))[np.newaxis, :, :]
        gt_boxes[:, 7:9] = common_utils.rotate_points_along_z(vel, angle)[0][:, 0:2]
    return (gt_boxes, points, noise_rotation) if return_rot else (gt_boxes, points)


def global_scaling(gt_boxes, points, scale_range, return_scale=False):
    if scale_range[1] - scale_range[0] < 1e-3:
        return (gt_boxes, points, 1.0) if return_scale else (gt_boxes, points)
    noise_scale = np.random.uniform(scale_range[0], scale_range[1])
    if _on_device(points):
        from .... import ops
        points = ops.points_world_transform(points.contiguous(), scale=np.float32(noise_scale))
    else:
        points[:, :3] *= noise_scale
    gt_boxes[:, :6] *= noise_scale
    return (gt_boxes, points, noise_scale) if return_scale else (gt_boxes, points)


def get_points_in_box(points, gt_box):
    """Points inside one box, margin 0.1 m in x / y, none in z, borders included (reference augmentor_utils.py:474-491).
    Host numpy; the device form of the same test is ops.points_in_boxes(mode=1)."""
    import math
    x, y, z = points[:, 0], points[:, 1], points[:, 2]
    cx, cy, cz, dx, dy, dz, rz = (gt_box[i] for i in range(7))
    sx, sy, sz = x - cx, y - cy, z - cz
    cosa, sina = math.cos(-rz), math.sin(-rz)
    lx = sx * cosa + sy * (-sina)
    ly = sx * sina + sy * cosa
    mask = np.logical_and(abs(sz) <= dz / 2.0, np.logical_and(abs(lx) <= dx / 2.0 + 1e-1, abs(ly) <= dy / 2.0 + 1e-1))
    return points[mask], mask


# ---------------------------------------------------------------------------------------------------------------------
# Per-object and pyramid augmentations (reference augmentor_utils.py:124-683), same names, same random draws in the same
# order.  numpy clouds keep the reference's numpy expressions.  CUDA clouds: the draws and the box updates stay on the host,
# a *_steps builder turns them into the step table of ops.points_box_steps, and one launch carries every point through the
# whole box list (a box changes only in its own iteration, after its mask was taken, so the boxes in the table do not
# depend on the points and the chain is exact).  Dropouts compact with the stable row select, so survivors keep their order.
_AXIS = {"x": 0, "y": 1, "z": 2}
_DROP = {"top": ("drop_z_ge", 2), "bottom": ("drop_z_le", 2), "left": ("drop_y_ge", 1), "right": ("drop_y_le", 1)}


def _step(box, op, p0=0.0, p1=0.0, world=False):
    from .... import ops
    row = np.zeros(ops.STEP_COLS, np.float64)
    if box is not None:
        row[:7] = box[:7]
    row[7] = ops.STEP_OPS[op] | (ops.STEP_WORLD if world else 0)
    row[8], row[9] = p0, p1
    return row


def _table(rows):
    from .... import ops
    return np.asarray(rows, np.float64).reshape(-1, ops.STEP_COLS)


def _run_steps(points, steps):
    """The device road of every function below: one launch; tables with a drop op are compacted in order."""
    from .... import ops
    points = points.contiguous()
    if len(steps) == 0:
        return points
    res = ops.points_box_steps(points, steps)
    if isinstance(res, tuple):
        return ops.RowBuffer(points.shape[0], points.shape[1], points.device).append(res[0], res[1], 1).finish()
    return res


def world_translation_steps(gt_boxes, offset_std, axis):
    """One draw (np.random.normal(0, std, 1), an fp64 array: numpy adds it in fp64 and rounds once); moves the boxes."""
    offset = np.random.normal(0, offset_std, 1)
    gt_boxes[:, _AXIS[axis]] += offset
    return _table([_step(None, "t" + axis, float(offset[0]), world=True)])


def local_translation_steps(gt_boxes, offset_range, axis):
    a, rows = _AXIS[axis], []
    for idx, box in enumerate(gt_boxes):
        offset = np.random.uniform(offset_range[0], offset_range[1])
        rows.append(_step(box, "t" + axis, float(np.float32(offset))))      # the table holds the box as it is tested
        gt_boxes[idx, a] += offset
    return _table(rows)


def local_rotation_steps(gt_boxes, rot_range):
    rows = []
    for idx, box in enumerate(gt_boxes):
        noise_rotation = np.random.uniform(rot_range[0], rot_range[1])
        a = torch.from_numpy(np.array([noise_rotation])).float()               # fp32 cos / sin of the fp32 angle
        rows.append(_step(box, "rot", float(torch.cos(a)), float(torch.sin(a))))
        _rotate_box(gt_boxes, idx, noise_rotation)
    return _table(rows)


def local_scaling_steps(gt_boxes, scale_range):
    rows = []
    if scale_range[1] - scale_range[0] < 1e-3:
        return _table(rows)
    for idx, box in enumerate(gt_boxes):
        noise_scale = np.random.uniform(scale_range[0], scale_range[1])
        rows.append(_step(box, "scale", float(np.float32(noise_scale))))
        gt_boxes[idx, 3:6] *= noise_scale
    return _table(rows)


def _local_threshold(box, intensity, direction):
    """(z + dz / 2) - intensity * dz and its three siblings, in the arithmetic of the boxes' dtype."""
    centre, size = (box[2], box[5]) if direction in ("top", "bottom") else (box[1], box[4])
    if direction in ("top", "left"):
        return (centre + size / 2) - intensity * size
    return (centre - size / 2) + intensity * size


def local_frustum_dropout_steps(gt_boxes, intensity_range, direction):
    rows = []
    for box in gt_boxes:
        intensity = np.random.uniform(intensity_range[0], intensity_range[1])
        rows.append(_step(box, _DROP[direction][0], float(_local_threshold(box, intensity, direction))))
    return _table(rows)


def _rotate_box(gt_boxes, idx, noise_rotation):
    """What local_rotation leaves of box idx: the centre is the pivot and stays, the heading turns.  The reference's velocity
    update (augmentor_utils.py:385-389) stacks a [2] row on an [N, 1] column and raises for boxes with velocity columns; here
    the box's own velocity is rotated, as global_rotation does for all boxes."""
    gt_boxes[idx, 6] += noise_rotation
    if gt_boxes.shape[1] > 8:
        vel = np.hstack((gt_boxes[idx, 7:9], np.zeros(1, gt_boxes.dtype)))[np.newaxis, np.newaxis, :]
        gt_boxes[idx, 7:9] = common_utils.rotate_points_along_z(vel, np.array([noise_rotation]))[0, 0, 0:2]


def _translation(gt_boxes, points, axis, arg, local):
    if _on_device(points):
        build = local_translation_steps if local else world_translation_steps
        return gt_boxes, _run_steps(points, build(gt_boxes, arg, axis))
    a = _AXIS[axis]
    if not local:
        offset = np.random.normal(0, arg, 1)
        points[:, a] += offset
        gt_boxes[:, a] += offset
        return gt_boxes, points
    for idx, box in enumerate(gt_boxes):
        offset = np.random.uniform(arg[0], arg[1])
        _, mask = get_points_in_box(points, box)
        points[mask, a] += offset
        gt_boxes[idx, a] += offset
    return gt_boxes, points


def random_translation_along_x(gt_boxes, points, offset_std):
    return _translation(gt_boxes, points, "x", offset_std, local=False)


def random_translation_along_y(gt_boxes, points, offset_std):
    return _translation(gt_boxes, points, "y", offset_std, local=False)


def random_translation_along_z(gt_boxes, points, offset_std):
    return _translation(gt_boxes, points, "z", offset_std, local=False)


def random_local_translation_along_x(gt_boxes, points, offset_range):
    return _translation(gt_boxes, points, "x", offset_range, local=True)


def random_local_translation_along_y(gt_boxes, points, offset_range):
    return _translation(gt_boxes, points, "y", offset_range, local=True)


def random_local_translation_along_z(gt_boxes, points, offset_range):
    return _translation(gt_boxes, points, "z", offset_range, local=True)


def local_scaling(gt_boxes, points, scale_range):
    if _on_device(points):
        return gt_boxes, _run_steps(points, local_scaling_steps(gt_boxes, scale_range))
    if scale_range[1] - scale_range[0] < 1e-3:
        return gt_boxes, points
    for idx, box in enumerate(gt_boxes):
        noise_scale = np.random.uniform(scale_range[0], scale_range[1])
        _, mask = get_points_in_box(points, box)
        for a in range(3):
            points[mask, a] -= box[a]
        points[mask, :3] *= noise_scale
        for a in range(3):
            points[mask, a] += box[a]
        gt_boxes[idx, 3:6] *= noise_scale
    return gt_boxes, points


def local_rotation(gt_boxes, points, rot_range):
    if _on_device(points):
        return gt_boxes, _run_steps(points, local_rotation_steps(gt_boxes, rot_range))
    for idx, box in enumerate(gt_boxes):
        noise_rotation = np.random.uniform(rot_range[0], rot_range[1])
        _, mask = get_points_in_box(points, box)
        centre = [box[0], box[1], box[2]]
        for a in range(3):
            points[mask, a] -= centre[a]
        points[mask, :] = common_utils.rotate_points_along_z(points[np.newaxis, mask, :], np.array([noise_rotation]))[0]
        for a in range(3):
            points[mask, a] += centre[a]
        _rotate_box(gt_boxes, idx, noise_rotation)
    return gt_boxes, points


def _global_frustum_dropout(gt_boxes, points, intensity_range, direction, return_mask):
    """threshold = max - intensity * (max - min) (top / left) or min + intensity * (max - min) (bottom / right) of z / y, in
    fp32 as numpy forms it; points and boxes on the far side go.  Device clouds: the extrema come from one reduction
    (ops.points_column_range, read back: the boxes are filtered on the host by the same threshold)."""
    col = _DROP[direction][1]
    intensity = np.random.uniform(intensity_range[0], intensity_range[1])
    dev = _on_device(points)
    if dev:
        from .... import ops
        points = points.contiguous()
        lo, hi = ops.points_column_range(points, col).cpu().numpy()
    else:
        hi, lo = np.max(points[:, col]), np.min(points[:, col])
    upper = direction in ("top", "left")
    threshold = hi - intensity * (hi - lo) if upper else lo + intensity * (hi - lo)
    if dev:
        points = _run_steps(points, _table([_step(None, _DROP[direction][0], float(threshold), world=True)]))
    else:
        points = points[points[:, col] < threshold] if upper else points[points[:, col] > threshold]
    keep = gt_boxes[:, col] < threshold if upper else gt_boxes[:, col] > threshold
    gt_boxes = gt_boxes[keep]
    return (gt_boxes, points, keep) if return_mask else (gt_boxes, points)


def global_frustum_dropout_top(gt_boxes, points, intensity_range, return_mask=False):
    return _global_frustum_dropout(gt_boxes, points, intensity_range, "top", return_mask)


def global_frustum_dropout_bottom(gt_boxes, points, intensity_range, return_mask=False):
    return _global_frustum_dropout(gt_boxes, points, intensity_range, "bottom", return_mask)


def global_frustum_dropout_left(gt_boxes, points, intensity_range, return_mask=False):
    return _global_frustum_dropout(gt_boxes, points, intensity_range, "left", return_mask)


def global_frustum_dropout_right(gt_boxes, points, intensity_range, return_mask=False):
    return _global_frustum_dropout(gt_boxes, points, intensity_range, "right", return_mask)


def _local_frustum_dropout(gt_boxes, points, intensity_range, direction):
    if _on_device(points):
        return gt_boxes, _run_steps(points, local_frustum_dropout_steps(gt_boxes, intensity_range, direction))
    col = _DROP[direction][1]
    for box in gt_boxes:
        intensity = np.random.uniform(intensity_range[0], intensity_range[1])
        _, mask = get_points_in_box(points, box)
        threshold = _local_threshold(box, intensity, direction)
        beyond = points[:, col] >= threshold if direction in ("top", "left") else points[:, col] <= threshold
        points = points[np.logical_not(np.logical_and(mask, beyond))]
    return gt_boxes, points


def local_frustum_dropout_top(gt_boxes, points, intensity_range):
    return _local_frustum_dropout(gt_boxes, points, intensity_range, "top")


def local_frustum_dropout_bottom(gt_boxes, points, intensity_range):
    return _local_frustum_dropout(gt_boxes, points, intensity_range, "bottom")


def local_frustum_dropout_left(gt_boxes, points, intensity_range):
    return _local_frustum_dropout(gt_boxes, points, intensity_range, "left")


def local_frustum_dropout_right(gt_boxes, points, intensity_range):
    return _local_frustum_dropout(gt_boxes, points, intensity_range, "right")


# ---- SE-SSD's shape-aware augmentation: the six pyramids apex = box centre, base = one face -----------------------------
_PYRAMID_FACES = ((0, 1, 5, 4), (4, 5, 6, 7), (7, 6, 2, 3), (3, 2, 1, 0), (1, 2, 6, 5), (0, 4, 7, 3))


def get_pyramids(boxes):
    """[N, 6, 15]: per face the box centre and the face's four corners in order round it (reference :494-516)."""
    from ...utils import box_utils
    corners = box_utils.boxes_to_corners_3d(boxes)                                        # [N, 8, 3]
    n = boxes.shape[0]
    apex = np.broadcast_to(boxes[:, None, None, 0:3], (n, 6, 1, 3))
    return np.concatenate((apex, corners[:, np.asarray(_PYRAMID_FACES)]), axis=2).reshape(n, 6, 15)


def pyramid_planes(pyramids):
    """[P, 5, 4] fp64 (nx, ny, nz, d): the five faces as half-spaces n . p <= d with outward normals - the four sides
    through the apex, then the base.  The same construction as the kernel's."""
    v = np.asarray(pyramids, np.float64).reshape(-1, 5, 3)
    g = v.sum(1) / 5.0
    a = np.concatenate((np.repeat(v[:, 0:1], 4, 1), v[:, 1:2]), 1)
    b = np.concatenate((v[:, 1:5], v[:, 2:3]), 1)
    e = np.concatenate((v[:, [2, 3, 4, 1]], v[:, 4:5]), 1)
    nrm = np.cross(b - a, e - a)
    nrm = np.where(((g[:, None] - a) * nrm).sum(-1, keepdims=True) > 0, -nrm, nrm)
    return np.concatenate((nrm, (nrm * a).sum(-1, keepdims=True)), -1)


def points_in_pyramids_mask(points, pyramids):
    """bool [n, P]: point inside pyramid (faces included).  The reference asks scipy's Delaunay hull (box_utils.in_hull) per
    pyramid; a pyramid is convex, so five half-space tests give the same answer away from the faces.  CUDA clouds:
    ops.points_in_pyramids, unpacked to a bool tensor."""
    pyramids = np.asarray(pyramids).reshape(-1, 5, 3)
    if _on_device(points):
        from .... import ops
        bits, _ = ops.points_in_pyramids(points.contiguous(), pyramids)
        p = torch.arange(pyramids.shape[0], device=points.device)
        return ((bits[:, p // 32] >> (p % 32)[None, :]) & 1).bool()
    flags = np.zeros((points.shape[0], pyramids.shape[0]), dtype=bool)
    xyz = points[:, 0:3].astype(np.float64)
    for i, pl in enumerate(pyramid_planes(pyramids)):
        flags[:, i] = (xyz @ pl[:, :3].T <= pl[None, :, 3]).all(-1)
    return flags


def _membership(points, pyramids):
    """(masks, counts): masks is the bool [n, P] array on the host road and the packed words on the device road - read
    through _members / _outside -, counts a host int array [P] (a read-back on the device road; _outside's compaction and
    each _members gather read a row count back too)."""
    pyramids = np.asarray(pyramids).reshape(-1, 5, 3)
    if _on_device(points):
        from .... import ops
        bits, counts = ops.points_in_pyramids(points, pyramids)
        return bits, counts.cpu().numpy().astype(np.int64)
    masks = points_in_pyramids_mask(points, pyramids)
    return masks, masks.sum(0)


def _members(points, masks, p):
    """Rows of pyramid p, in order (device road: torch.nonzero, which reads the row count back)."""
    if _on_device(points):
        from .... import ops
        return points[torch.nonzero(ops.pyramid_bit(masks, p)).squeeze(1)]
    return points[masks[:, p]]


def _outside(points, masks, which):
    """Rows in none of the pyramids `which` (bool [P]), in order."""
    if _on_device(points):
        from .... import ops
        words = np.zeros(masks.shape[1] * 32, np.uint32)
        words[:len(which)] = which
        words = (words.reshape(-1, 32) << np.arange(32, dtype=np.uint32)).sum(1, dtype=np.uint32).view(np.int32)
        hit = ((masks & torch.from_numpy(words).to(masks.device)[None, :]) != 0).any(1).to(torch.int32)
        return ops.RowBuffer(points.shape[0], points.shape[1], points.device).append(points, hit, 0).finish()
    return points[np.logical_not(masks[:, which].any(-1))]


def _cat(points, parts):
    return torch.cat(parts, dim=0) if _on_device(points) else np.concatenate(parts, axis=0)


def _one_face_per_box(n_boxes, prob):
    """The draws local_pyramid_dropout and _sparsify share: a face per box, then which boxes take part."""
    face = np.random.randint(0, 6, (n_boxes))
    return face, np.random.uniform(0, 1, (n_boxes)) <= prob


def local_pyramid_dropout(gt_boxes, points, dropout_prob, pyramids=None):
    if pyramids is None:
        pyramids = get_pyramids(gt_boxes).reshape([-1, 6, 5, 3])
    face, drop_box_mask = _one_face_per_box(pyramids.shape[0], dropout_prob)
    if np.sum(drop_box_mask) != 0:
        drop_pyramids = pyramids[drop_box_mask, face[drop_box_mask]]
        if _on_device(points):
            points = points.contiguous()
        masks, _ = _membership(points, drop_pyramids)
        points = _outside(points, masks, np.ones(drop_pyramids.shape[0], bool))
    return gt_boxes, points, pyramids[np.logical_not(drop_box_mask)]


def local_pyramid_sparsify(gt_boxes, points, prob, max_num_pts, pyramids=None):
    if pyramids is None:
        pyramids = get_pyramids(gt_boxes).reshape([-1, 6, 5, 3])
    if pyramids.shape[0] > 0:
        face, sparsify_box_mask = _one_face_per_box(pyramids.shape[0], prob)
        sampled = pyramids[sparsify_box_mask, face[sparsify_box_mask]]
        if _on_device(points):
            points = points.contiguous()
        masks, counts = _membership(points, sampled)
        valid = counts > max_num_pts                                   # only pyramids that hold more are thinned
        if valid.sum() > 0:
            parts = [_outside(points, masks, valid)]
            for p in np.nonzero(valid)[0]:
                chosen = np.random.choice(int(counts[p]), size=max_num_pts, replace=False)
                sample = _members(points, masks, p)
                parts.append(sample[torch.from_numpy(chosen).to(points.device)] if _on_device(points) else sample[chosen])
            points = _cat(points, parts)
        pyramids = pyramids[np.logical_not(sparsify_box_mask)]
    return gt_boxes, points, pyramids


def _sum3(t):
    """Sum over a last axis of three in numpy's order, (a + b) + c, whatever the backend's reduction does."""
    return (t[..., 0] + t[..., 1]) + t[..., 2]


def _pyramid_frame(pyramid):
    """Base corner 0, the two base edges from it, the base centre and the axis from there to the apex (15 values)."""
    origin = pyramid[3:6]
    centre = (pyramid[3:6] + pyramid[6:9] + pyramid[9:12] + pyramid[12:]) / 4.0
    return origin, pyramid[6:9] - origin, pyramid[12:] - origin, centre, pyramid[0:3] - centre


def _points_ratio(points, pyramid):
    origin, v0, v1, centre, v2 = _pyramid_frame(pyramid)
    alphas = _sum3((points[:, 0:3] - origin) * v0) / _sum3(v0 ** 2)
    betas = _sum3((points[:, 0:3] - origin) * v1) / _sum3(v1 ** 2)
    gammas = _sum3((points[:, 0:3] - centre) * v2) / _sum3(v2 ** 2)
    return alphas, betas, gammas


def _recover_points(ratio, pyramid):
    alphas, betas, gammas = ratio
    origin, v0, v1, _, v2 = _pyramid_frame(pyramid)
    return (alphas[:, None] * v0 + betas[:, None] * v1) + origin + gammas[:, None] * v2


def _intensity_ratio(col):
    lo, hi = col.min(), col.max()
    return (col - lo) / (hi - lo).clip(1e-6, 1), lo, hi


def _swap_pair(a_points, b_points, a_pyramid, b_pyramid):
    """The points of pyramid b placed in a at their relative positions, and the other way round; the last column (intensity)
    is mapped through the two ranges.  Works on numpy arrays and on torch tensors alike."""
    a_int, a_lo, a_hi = _intensity_ratio(a_points[:, -1:])
    b_int, b_lo, b_hi = _intensity_ratio(b_points[:, -1:])
    new_a = _recover_points(_points_ratio(b_points, b_pyramid), a_pyramid)
    new_b = _recover_points(_points_ratio(a_points, a_pyramid), b_pyramid)
    return new_a, b_int * (a_hi - a_lo) + a_lo, new_b, a_int * (b_hi - b_lo) + b_lo


def local_pyramid_swap(gt_boxes, points, prob, max_num_pts, pyramids=None):
    if pyramids is None:
        pyramids = get_pyramids(gt_boxes).reshape([-1, 6, 5, 3])
    n_boxes = pyramids.shape[0]
    swap_box_mask = np.random.uniform(0, 1, (n_boxes)) <= prob
    if swap_box_mask.sum() == 0:
        return gt_boxes, points
    if points.shape[1] != 4:
        raise ValueError("local_pyramid_swap writes (x, y, z, intensity) rows: the cloud needs 4 columns")
    dev = _on_device(points)
    if dev:
        points = points.contiguous()
    _, counts = _membership(points, pyramids)
    filled = counts.reshape(n_boxes, -1) > max_num_pts                   # [N, 6]; dropped or occluded pyramids do not take part
    selected = filled * swap_box_mask[:, None]
    if selected.sum() == 0:
        return gt_boxes, points
    # one filled face of every chosen box ...
    index_i, index_j = np.nonzero(selected)
    face = [np.random.choice(index_j[index_i == i]) if e and (index_i == i).any() else 0 for i, e in enumerate(swap_box_mask)]
    to_swap_mask = np.zeros_like(selected, dtype=bool)
    to_swap_mask[np.arange(n_boxes), face] = True
    to_swap_mask &= selected.astype(bool)
    to_swap = pyramids[to_swap_mask]
    # ... and for each a partner: the same face of another box where it is filled, else itself
    index_i, index_j = np.nonzero(to_swap_mask)
    filled[to_swap_mask] = False
    partner_i = np.array([np.random.choice(np.where(filled[:, j])[0]) if np.where(filled[:, j])[0].shape[0] > 0 else index_i[i]
                          for i, j in enumerate(index_j.tolist())])
    swapped = pyramids[partner_i.astype(np.int32), index_j.astype(np.int32)]
    pairs = swapped.shape[0]
    both = np.concatenate([to_swap, swapped], axis=0)
    masks, _ = _membership(points, both)
    parts = [_outside(points, masks, np.ones(2 * pairs, bool))]
    for i in range(pairs):
        a_pyr, b_pyr = to_swap[i].reshape(15), swapped[i].reshape(15)
        if dev:
            a_pyr, b_pyr = torch.from_numpy(a_pyr).to(points.device), torch.from_numpy(b_pyr).to(points.device)
        new_a, int_a, new_b, int_b = _swap_pair(_members(points, masks, i), _members(points, masks, i + pairs), a_pyr, b_pyr)
        if dev:
            parts += [torch.cat([new_a, int_a], dim=1).to(points.dtype), torch.cat([new_b, int_b], dim=1).to(points.dtype)]
        else:
            parts += [np.concatenate([new_a, int_a], axis=1), np.concatenate([new_b, int_b], axis=1)]
    return gt_boxes, _cat(points, parts)
