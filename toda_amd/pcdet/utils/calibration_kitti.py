"""KITTI camera calibration (behaviour of reference pcdet/utils/calibration_kitti.py): the P2 / R0_rect / Tr_velo_to_cam
matrices of a calib file and the LiDAR <-> rectified camera <-> image maps built from them, in numpy fp32.

These maps act on annotation boxes (a few hundred rows per frame at most) and on host arrays that end up in annotation dicts.
The per-point field-of-view test of a whole frame does not go through them: it runs on the device from `fov_matrices()`
(toda_amd.ops.points_fov_flags, csrc/kitti_frame.hip)."""
import numpy as np

_ROWS = {"P2": (2, (3, 4)), "P3": (3, (3, 4)), "R0": (4, (3, 3)), "Tr_velo2cam": (5, (3, 4))}


def get_calib_from_file(calib_file):
    """Lines 2-5 of a KITTI calib file ("P2: ...", "P3: ...", "R0_rect: ...", "Tr_velo_to_cam: ...") as fp32 matrices."""
    with open(calib_file) as f:
        lines = f.readlines()
    return {key: np.array(lines[row].strip().split(" ")[1:], dtype=np.float32).reshape(shape) for key, (row, shape) in _ROWS.items()}


def _with_ones(pts):
    return np.hstack((pts, np.ones((pts.shape[0], 1), dtype=np.float32)))


class Calibration:
    def __init__(self, calib_file):
        calib = calib_file if isinstance(calib_file, dict) else get_calib_from_file(calib_file)
        self.P2 = calib["P2"]               # 3 x 4
        self.R0 = calib["R0"]               # 3 x 3
        self.V2C = calib["Tr_velo2cam"]     # 3 x 4
        self.cu, self.cv = self.P2[0, 2], self.P2[1, 2]
        self.fu, self.fv = self.P2[0, 0], self.P2[1, 1]
        self.tx, self.ty = self.P2[0, 3] / (-self.fu), self.P2[1, 3] / (-self.fv)

    def cart_to_hom(self, pts):
        return _with_ones(pts)

    def lidar_to_rect_matrix(self):
        """[4, 3]: rect = [x y z 1] . M, the product the reference forms on every call."""
        return np.dot(self.V2C.T, self.R0.T)

    def fov_matrices(self):
        """(M [4, 3], P2 [3, 4]) as contiguous fp32, the two by-value arguments of ops.points_fov_flags."""
        return (np.ascontiguousarray(self.lidar_to_rect_matrix(), dtype=np.float32), np.ascontiguousarray(self.P2, dtype=np.float32))

    def lidar_to_rect(self, pts_lidar):
        return np.dot(_with_ones(pts_lidar), self.lidar_to_rect_matrix())

    def rect_to_lidar(self, pts_rect):
        r0 = np.zeros((4, 4), dtype=np.float32)
        r0[:3, :3], r0[3, 3] = self.R0, 1
        v2c = np.zeros((4, 4), dtype=np.float32)
        v2c[:3, :], v2c[3, 3] = self.V2C, 1
        return np.dot(_with_ones(pts_rect), np.linalg.inv(np.dot(r0, v2c).T))[:, 0:3]

    def rect_to_img(self, pts_rect):
        """-> (pixels [N, 2], depth [N]): homogeneous projection by P2, divided by the rectified z."""
        hom = _with_ones(pts_rect)
        proj = np.dot(hom, self.P2.T)
        return (proj[:, 0:2].T / hom[:, 2]).T, proj[:, 2] - self.P2.T[3, 2]

    def lidar_to_img(self, pts_lidar):
        return self.rect_to_img(self.lidar_to_rect(pts_lidar))

    def img_to_rect(self, u, v, depth_rect):
        x = ((u - self.cu) * depth_rect) / self.fu + self.tx
        y = ((v - self.cv) * depth_rect) / self.fv + self.ty
        return np.stack([x.reshape(-1), y.reshape(-1), depth_rect.reshape(-1)], axis=1)

    def corners3d_to_img_boxes(self, corners3d):
        """corners3d [N, 8, 3] in the rectified frame -> (boxes [N, 4] x1 y1 x2 y2, their corners' pixels [N, 8, 2])."""
        hom = np.concatenate((corners3d, np.ones((corners3d.shape[0], 8, 1))), axis=2)
        proj = np.matmul(hom, self.P2.T)
        x, y = proj[:, :, 0] / proj[:, :, 2], proj[:, :, 1] / proj[:, :, 2]
        boxes = np.stack([x.min(axis=1), y.min(axis=1), x.max(axis=1), y.max(axis=1)], axis=1)
        return boxes, np.stack([x, y], axis=2)
