"""LiDAR-frame annotations in the KITTI annotation layout (reference pcdet/datasets/kitti/kitti_utils.py), the route by
which datasets without cameras reach the KITTI evaluator: no calibration, a constant placeholder image box."""
import numpy as np

PLACEHOLDER_IMAGE_BOX = (0.0, 0.0, 50.0, 50.0)      # 50 px tall: above the minimum height of every difficulty


def _camera_fields(boxes, fakelidar):
    """[n, 7] LiDAR boxes (x, y, z, dx, dy, dz, heading; z at the centre) -> location, dimensions, rotation_y, alpha.
    Camera axes: x_cam = -y, y_cam = -(bottom face height), z_cam = x; dimensions are l, h, w."""
    x, y, z, dx, dy, dz, heading = (boxes[:, k] for k in range(7))
    if fakelidar:                                   # older layout: z at the bottom face, then w, l, h and the camera angle
        z, dx, dy, heading = z + dz / 2, dy, dx, -(heading + np.pi / 2)
    bottom = z - dz / 2
    rotation_y = -heading - np.pi / 2.0
    return {"location": np.stack([-y, -bottom, x], axis=1), "dimensions": np.stack([dx, dz, dy], axis=1),
            "rotation_y": rotation_y, "alpha": -np.arctan2(-y, x) + rotation_y}


def transform_annotations_to_kitti_format(annos, map_name_to_kitti=None, info_with_fakelidar=False):
    """In place, per anno: names (`name`, or `gt_names` moved to `name`) mapped through map_name_to_kitti inside their own
    array; bbox the placeholder, truncated = occluded = 0; boxes_lidar / gt_boxes_lidar -> location, dimensions,
    rotation_y = -heading - pi / 2, alpha."""
    for anno in annos:
        names = anno["name"] if "name" in anno else anno.pop("gt_names")
        names[:] = [map_name_to_kitti[n] for n in names]
        count = len(names)
        anno["name"] = names
        anno["bbox"] = np.tile(np.array(PLACEHOLDER_IMAGE_BOX), (count, 1))
        anno["truncated"], anno["occluded"] = np.zeros(count), np.zeros(count)
        boxes = np.array(anno["boxes_lidar"] if "boxes_lidar" in anno else anno["gt_boxes_lidar"], copy=True)
        if len(boxes):
            anno.update(_camera_fields(boxes, info_with_fakelidar))
        else:
            anno.update(location=np.zeros((0, 3)), dimensions=np.zeros((0, 3)), rotation_y=np.zeros(0), alpha=np.zeros(0))
    return annos
