"""One line of a KITTI label file (behaviour of reference pcdet/utils/object3d_kitti.py): type, truncation, occlusion, alpha,
the 2D box, h w l, the location in the rectified camera frame, rotation_y, an optional score, and the difficulty level the
benchmark derives from box height, truncation and occlusion."""
import numpy as np

_CLS_ID = {"Car": 1, "Pedestrian": 2, "Cyclist": 3, "Van": 4}
# (name, level, min 2D height, max truncation, max occlusion), first match wins
_LEVELS = (("Easy", 0, 40, 0.15, 0), ("Moderate", 1, 25, 0.3, 1), ("Hard", 2, 25, 0.5, 2))


def get_objects_from_label(label_file):
    with open(label_file, "r") as f:
        return [Object3d(line) for line in f.readlines()]


def cls_type_to_id(cls_type):
    return _CLS_ID.get(cls_type, -1)


class Object3d:
    def __init__(self, line):
        field = line.strip().split(" ")
        self.src = line
        self.cls_type = field[0]
        self.cls_id = cls_type_to_id(self.cls_type)
        self.truncation = float(field[1])
        self.occlusion = float(field[2])        # 0 visible, 1 partly, 2 largely occluded, 3 unknown
        self.alpha = float(field[3])
        self.box2d = np.array([float(v) for v in field[4:8]], dtype=np.float32)
        self.h, self.w, self.l = float(field[8]), float(field[9]), float(field[10])
        self.loc = np.array([float(v) for v in field[11:14]], dtype=np.float32)
        self.dis_to_cam = np.linalg.norm(self.loc)
        self.ry = float(field[14])
        self.score = float(field[15]) if len(field) == 16 else -1.0
        self.level_str = None
        self.level = self.get_kitti_obj_level()

    def get_kitti_obj_level(self):
        height = float(self.box2d[3]) - float(self.box2d[1]) + 1
        for name, level, min_height, max_trunc, max_occ in _LEVELS:
            if height >= min_height and self.truncation <= max_trunc and self.occlusion <= max_occ:
                self.level_str = name
                return level
        self.level_str = "UnKnown"
        return -1

    def generate_corners3d(self):
        """[8, 3] corners in the camera frame: the bottom face (y = loc_y) first, then the top, turned by ry about y."""
        hl, hw = self.l / 2, self.w / 2
        local = np.array([[hl, hl, -hl, -hl, hl, hl, -hl, -hl], [0, 0, 0, 0, -self.h, -self.h, -self.h, -self.h],
                          [hw, -hw, -hw, hw, hw, -hw, -hw, hw]])
        c, s = np.cos(self.ry), np.sin(self.ry)
        return np.dot(np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]]), local).T + self.loc

    def to_str(self):
        return "%s %.3f %.3f %.3f box2d: %s hwl: [%.3f %.3f %.3f] pos: %s ry: %.3f" % (
            self.cls_type, self.truncation, self.occlusion, self.alpha, self.box2d, self.h, self.w, self.l, self.loc, self.ry)

    def to_kitti_format(self):
        return "%s %.2f %d %.2f %.2f %.2f %.2f %.2f %.2f %.2f %.2f %.2f %.2f %.2f %.2f" % (
            self.cls_type, self.truncation, int(self.occlusion), self.alpha, *self.box2d, self.h, self.w, self.l, *self.loc, self.ry)
