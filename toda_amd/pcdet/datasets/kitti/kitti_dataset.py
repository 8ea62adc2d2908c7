"""KittiDataset (behaviour of reference pcdet/datasets/kitti/kitti_dataset.py): the KITTI object benchmark on disk ->
training / evaluation samples, info pickles, the GT-sampling database, camera-frame prediction dicts, result files and the
official AP.

    <root>/ImageSets/{train,val,test}.txt
    <root>/{training,testing}/{velodyne/*.bin, label_2/*.txt, calib/*.txt, image_2/*.png, planes/*.txt}

MI355X layout: the frame's points go file -> one H2D copy -> camera field-of-view flags (ops.points_fov_flags,
csrc/kitti_frame.hip) -> stable compaction (ops.RowBuffer) -> SHIFT_COOR (a tensor add) and then, still on the device, the
range mask, the shuffle and the voxeliser of the data processor.  With FOV_POINTS_ONLY the samples are CUDA tensors
(`on_device`): build_dataloader then runs the dataset in the training process (num_workers = 0), no worker process opens the
GPU.  Without it the points stay numpy and reach the device with the batch, as SyntheticLidarDataset's do; raw_frame(device=True),
the frame before prepare_data that NusKittiMixDataset mixes, uploads them in either setting.  The info
builder counts the points of every gt box on the device as well (points_in_boxes mode 2 + bincount) where the reference
runs one Delaunay hull test per box.  Label, calibration and box arithmetic are host numpy.

Images, depth maps and the calibration matrices of CaDDN are out of scope: naming them in GET_ITEM_LIST is an error.

    python -m toda_amd.pcdet.datasets.kitti.kitti_dataset create_kitti_infos <dataset yaml> [--data_path DIR]
"""
import copy
import pickle
import struct
from pathlib import Path

import numpy as np
import torch

from ...utils import box_utils, calibration_kitti, common_utils, object3d_kitti
from ..dataset import DatasetTemplate

_OUT_OF_SCOPE_ITEMS = ("images", "depth_maps", "calib_matricies")
_PNG_MAGIC = b"\x89PNG\r\n\x1a\n"


def png_image_shape(path):
    """(height, width) int32 from the first 24 bytes of a PNG: the 8-byte signature, the IHDR chunk's length and tag, then
    width and height as big-endian uint32.  No imaging library."""
    with open(path, "rb") as f:
        head = f.read(24)
    if len(head) < 24 or head[:8] != _PNG_MAGIC or head[12:16] != b"IHDR":
        raise ValueError(f"{path} is not a PNG file")
    width, height = struct.unpack(">II", head[16:24])
    return np.array([height, width], dtype=np.int32)


class KittiDataset(DatasetTemplate):
    def __init__(self, dataset_cfg, class_names, training=True, root_path=None, logger=None):
        super().__init__(dataset_cfg=dataset_cfg, class_names=class_names, training=training, root_path=root_path, logger=logger)
        self.root_path = Path(self.root_path)
        self.get_item_list = list(dataset_cfg.get("GET_ITEM_LIST", ["points"]))
        for item in self.get_item_list:
            if item in _OUT_OF_SCOPE_ITEMS:
                raise NotImplementedError(f"GET_ITEM_LIST entry '{item}' feeds CaDDN's image branch, which is out of scope: "
                                          "KittiDataset serves points, gt_boxes2d, calib and image_shape")
        self.fov_points_only = bool(dataset_cfg.get("FOV_POINTS_ONLY", False))
        self.shift_coor = dataset_cfg.get("SHIFT_COOR", None)
        # samples leave __getitem__ as CUDA tensors: build_dataloader keeps such a dataset in the training process
        self.on_device = self.fov_points_only and "points" in self.get_item_list
        self.set_split(dataset_cfg.DATA_SPLIT[self.mode])
        self.kitti_infos = []
        self.include_kitti_data(self.mode)

    # ---- reading
    def include_kitti_data(self, mode):
        if self.logger is not None:
            self.logger.info("Loading KITTI dataset")
        loaded = []
        for rel in self.dataset_cfg.INFO_PATH[mode]:
            path = self.root_path / rel
            if not path.exists():
                continue
            with open(path, "rb") as f:
                loaded.extend(pickle.load(f))
        self.kitti_infos.extend(loaded)
        if self.logger is not None:
            self.logger.info("Total samples for KITTI dataset: %d" % len(loaded))

    def set_split(self, split):
        self.split = split
        self.root_split_path = self.root_path / ("testing" if split == "test" else "training")
        listing = self.root_path / "ImageSets" / f"{split}.txt"
        self.sample_id_list = [line.strip() for line in open(listing).readlines()] if listing.exists() else None

    def _frame_file(self, folder, idx, suffix):
        path = self.root_split_path / folder / f"{idx}.{suffix}"
        assert path.exists(), path
        return path

    def get_lidar(self, idx):
        return np.fromfile(str(self._frame_file("velodyne", idx, "bin")), dtype=np.float32).reshape(-1, 4)

    def get_image_shape(self, idx):
        return png_image_shape(self._frame_file("image_2", idx, "png"))

    def get_label(self, idx):
        return object3d_kitti.get_objects_from_label(self._frame_file("label_2", idx, "txt"))

    def get_calib(self, idx):
        return calibration_kitti.Calibration(self._frame_file("calib", idx, "txt"))

    def get_road_plane(self, idx):
        """Unit normal and offset (a, b, c, d) of the frame's road plane in the rectified camera frame, the normal pointing
        up (-y); None when the frame has no plane file."""
        path = self.root_split_path / "planes" / f"{idx}.txt"
        if not path.exists():
            return None
        with open(path, "r") as f:
            plane = np.asarray([float(v) for v in f.readlines()[3].split()])
        if plane[1] > 0:
            plane = -plane
        return plane / np.linalg.norm(plane[0:3])

    @staticmethod
    def get_fov_flag(pts_rect, img_shape, calib):
        """The host form of the field-of-view test (numpy, for annotation-sized inputs and as the test oracle)."""
        pts_img, depth = calib.rect_to_img(pts_rect)
        in_u = np.logical_and(pts_img[:, 0] >= 0, pts_img[:, 0] < img_shape[1])
        in_v = np.logical_and(pts_img[:, 1] >= 0, pts_img[:, 1] < img_shape[0])
        return np.logical_and(np.logical_and(in_u, in_v), depth >= 0)

    def fov_points(self, points, calib, img_shape):
        """points [n, c] numpy -> the rows inside the camera image as a CUDA tensor, in order: one upload, one flag pass, one
        stable compaction."""
        from .... import ops
        pts = torch.from_numpy(np.ascontiguousarray(points, dtype=np.float32)).cuda()
        m, p2 = calib.fov_matrices()
        flags = ops.points_fov_flags(pts, m, p2, img_shape)
        return ops.RowBuffer(pts.shape[0], pts.shape[1], pts.device).append(pts, flags, 1).finish()

    # ---- infos
    def get_infos(self, num_workers=4, has_label=True, count_inside_pts=True, sample_id_list=None):
        """One record per frame in the reference's layout.  num_workers is accepted for signature parity: the frames are
        visited serially, the per-frame work is a few small files and (count_inside_pts) three launches."""
        return [self._frame_info(idx, has_label, count_inside_pts) for idx in (sample_id_list if sample_id_list is not None else self.sample_id_list)]

    def _frame_info(self, sample_idx, has_label, count_inside_pts):
        info = {"point_cloud": {"num_features": 4, "lidar_idx": sample_idx},
                "image": {"image_idx": sample_idx, "image_shape": self.get_image_shape(sample_idx)}}
        calib = self.get_calib(sample_idx)
        p2 = np.concatenate([calib.P2, np.array([[0.0, 0.0, 0.0, 1.0]])], axis=0)
        r0 = np.zeros([4, 4], dtype=calib.R0.dtype)
        r0[3, 3], r0[:3, :3] = 1.0, calib.R0
        v2c = np.concatenate([calib.V2C, np.array([[0.0, 0.0, 0.0, 1.0]])], axis=0)
        info["calib"] = {"P2": p2, "R0_rect": r0, "Tr_velo_to_cam": v2c}
        if not has_label:
            return info
        objs = self.get_label(sample_idx)
        annos = {"name": np.array([o.cls_type for o in objs]), "truncated": np.array([o.truncation for o in objs]),
                 "occluded": np.array([o.occlusion for o in objs]), "alpha": np.array([o.alpha for o in objs]),
                 "bbox": np.concatenate([o.box2d.reshape(1, 4) for o in objs], axis=0),
                 "dimensions": np.array([[o.l, o.h, o.w] for o in objs]),                      # l, h, w: the camera layout
                 "location": np.concatenate([o.loc.reshape(1, 3) for o in objs], axis=0),
                 "rotation_y": np.array([o.ry for o in objs]), "score": np.array([o.score for o in objs]),
                 "difficulty": np.array([o.level for o in objs], np.int32)}
        # the benchmark's label files list the DontCare regions last: the first num_objects entries are the objects
        num_objects, num_gt = sum(o.cls_type != "DontCare" for o in objs), len(objs)
        annos["index"] = np.array(list(range(num_objects)) + [-1] * (num_gt - num_objects), dtype=np.int32)
        loc, dims, rots = annos["location"][:num_objects], annos["dimensions"][:num_objects], annos["rotation_y"][:num_objects]
        loc_lidar = calib.rect_to_lidar(loc)
        loc_lidar[:, 2] += dims[:, 1] / 2
        annos["gt_boxes_lidar"] = np.concatenate([loc_lidar, dims[:, 0:1], dims[:, 2:3], dims[:, 1:2], -(np.pi / 2 + rots[..., np.newaxis])], axis=1)
        info["annos"] = annos
        if count_inside_pts:
            annos["num_points_in_gt"] = self._count_points_in_gt(sample_idx, calib, info["image"]["image_shape"], annos["gt_boxes_lidar"], num_gt)
        return info

    def _count_points_in_gt(self, sample_idx, calib, img_shape, gt_boxes_lidar, num_gt):
        """Points of the camera's field of view inside every gt box, -1 for the DontCare entries: on the device, the index of
        the box that holds each point (the roiaware test) and a bincount."""
        from .... import ops
        counts = -np.ones(num_gt, dtype=np.int32)
        k = gt_boxes_lidar.shape[0]
        if k == 0:
            return counts
        pts = self.fov_points(self.get_lidar(sample_idx), calib, img_shape)
        boxes = torch.from_numpy(np.ascontiguousarray(gt_boxes_lidar, dtype=np.float32)).cuda()
        owner = ops.points_in_boxes(pts.contiguous(), boxes, mode=2)
        counts[:k] = torch.bincount(owner[owner >= 0].long(), minlength=k).cpu().numpy()
        return counts

    def dump_infos(self, path):
        """The label-free view of the infos (no `annos`): what tools/generate_pseudo_labels fills with a teacher's detections."""
        with open(path, "wb") as f:
            pickle.dump([{k: v for k, v in info.items() if k != "annos"} for info in self.kitti_infos], f)

    # ---- GT database: the frames of an infos pickle through augmentor/database_sampler.create_groundtruth_database
    def create_groundtruth_database(self, info_path=None, used_classes=None, split="train"):
        from ..augmentor.database_sampler import create_groundtruth_database
        with open(info_path, "rb") as f:
            infos = pickle.load(f)
        return create_groundtruth_database(_InfoFrames(self, infos), self.root_path, used_classes=used_classes, packed=False,
                                           db_name="gt_database" if split == "train" else f"gt_database_{split}",
                                           info_name=f"kitti_dbinfos_{split}.pkl",
                                           frame_id=lambda k: infos[k]["point_cloud"]["lidar_idx"],
                                           extra_info=lambda k, i: {"difficulty": infos[k]["annos"]["difficulty"][i], "bbox": infos[k]["annos"]["bbox"][i],
                                                                    "score": infos[k]["annos"]["score"][i]})

    # ---- predictions
    def generate_prediction_dicts(self, batch_dict, pred_dicts, class_names, output_path=None):
        """Per frame: LiDAR boxes (SHIFT_COOR undone) -> camera boxes -> clipped image boxes -> the KITTI annotation dict
        (name, truncated, occluded, alpha, bbox, dimensions l h w, location, rotation_y, score, boxes_lidar, frame_id);
        with output_path also `<frame>.txt` in the submission format (type -1 -1 alpha bbox h w l x y z ry score)."""
        annos = []
        for index, box_dict in enumerate(pred_dicts):
            scores = box_dict["pred_scores"].detach().cpu().numpy()
            boxes = box_dict["pred_boxes"].detach().cpu().numpy()
            labels = box_dict["pred_labels"].detach().cpu().numpy().astype(np.int64)
            n = scores.shape[0]
            anno = {"name": np.zeros(n), "truncated": np.zeros(n), "occluded": np.zeros(n), "alpha": np.zeros(n), "bbox": np.zeros([n, 4]),
                    "dimensions": np.zeros([n, 3]), "location": np.zeros([n, 3]), "rotation_y": np.zeros(n), "score": np.zeros(n),
                    "boxes_lidar": np.zeros([n, 7])}
            if n:
                boxes = boxes[:, :7]
                if self.shift_coor:
                    boxes[:, 0:3] -= np.asarray(self.shift_coor, dtype=boxes.dtype)
                calib = batch_dict["calib"][index]
                shape = batch_dict["image_shape"][index]
                shape = shape.cpu().numpy() if torch.is_tensor(shape) else np.asarray(shape)
                cam = box_utils.boxes3d_lidar_to_kitti_camera(boxes, calib)
                anno.update(name=np.array(class_names)[labels - 1], alpha=-np.arctan2(-boxes[:, 1], boxes[:, 0]) + cam[:, 6],
                            bbox=box_utils.boxes3d_kitti_camera_to_imageboxes(cam, calib, image_shape=shape), dimensions=cam[:, 3:6],
                            location=cam[:, 0:3], rotation_y=cam[:, 6], score=scores, boxes_lidar=boxes)
            anno["frame_id"] = batch_dict["frame_id"][index]
            annos.append(anno)
            if output_path is not None:
                with open(Path(output_path) / f"{anno['frame_id']}.txt", "w") as f:
                    for k in range(n):
                        l, h, w = anno["dimensions"][k]
                        f.write("%s -1 -1 %.4f %.4f %.4f %.4f %.4f %.4f %.4f %.4f %.4f %.4f %.4f %.4f %.4f\n" % (
                            anno["name"][k], anno["alpha"][k], *anno["bbox"][k], h, w, l, *anno["location"][k], anno["rotation_y"][k], anno["score"][k]))
        return annos

    def evaluation(self, det_annos, class_names, **kwargs):
        """The official KITTI AP table (bbox / bev / 3d / aos, R11 and R40) of det_annos against the infos' annotations, both
        deep-copied; (None, {}) when the infos carry no annotations (the test split)."""
        if not self.kitti_infos or "annos" not in self.kitti_infos[0]:
            return None, {}
        from .kitti_object_eval_python import eval as kitti_eval
        gt_annos = [copy.deepcopy(info["annos"]) for info in self.kitti_infos]
        return kitti_eval.get_official_eval_result(gt_annos, copy.deepcopy(det_annos), class_names)

    # ---- samples
    def __len__(self):
        if self._merge_all_iters_to_one_epoch:
            return len(self.kitti_infos) * self.total_epochs
        return len(self.kitti_infos)

    def raw_frame(self, index, device=False):
        """Frame `index` of the infos before prepare_data: {frame_id, calib, image_shape}, with annotations gt_names / gt_boxes
        [n, 7] (DontCare dropped, camera -> LiDAR, SHIFT_COOR added), gt_boxes2d when GET_ITEM_LIST names it and road_plane when
        the frame has a plane file, and `points` when GET_ITEM_LIST names them.  device: the points are a CUDA tensor without
        FOV_POINTS_ONLY too (one upload; SHIFT_COOR is added after it in fp32, the bits of the host addition)."""
        info = copy.deepcopy(self.kitti_infos[index])
        sample_idx = info["point_cloud"]["lidar_idx"]
        img_shape = info["image"]["image_shape"]
        calib = self.get_calib(sample_idx)
        data = {"frame_id": sample_idx, "calib": calib, "image_shape": img_shape}
        if "annos" in info:
            annos = common_utils.drop_info_with_name(info["annos"], name="DontCare")
            cam = np.concatenate([annos["location"], annos["dimensions"], annos["rotation_y"][..., np.newaxis]], axis=1).astype(np.float32)
            data["gt_names"] = annos["name"]
            data["gt_boxes"] = box_utils.boxes3d_kitti_camera_to_lidar(cam, calib)
            if self.shift_coor:
                data["gt_boxes"][:, 0:3] += self.shift_coor
            if "gt_boxes2d" in self.get_item_list:
                data["gt_boxes2d"] = annos["bbox"]
            plane = self.get_road_plane(sample_idx)
            if plane is not None:
                data["road_plane"] = plane
        if "points" in self.get_item_list:
            points = self.get_lidar(sample_idx)
            if self.fov_points_only:
                points = self.fov_points(points, calib, img_shape)
            elif device:
                points = torch.from_numpy(np.ascontiguousarray(points, dtype=np.float32)).cuda()
            if self.shift_coor:
                shift = np.array(self.shift_coor, dtype=np.float32)
                points[:, 0:3] += torch.from_numpy(shift).to(points.device) if torch.is_tensor(points) else shift
            data["points"] = points
        return data

    def __getitem__(self, index):
        if self._merge_all_iters_to_one_epoch:
            index = index % len(self.kitti_infos)
        data = self.prepare_data(self.raw_frame(index))
        if self.training and data.get("gt_boxes") is not None and len(data["gt_boxes"]) == 0:      # reference dataset.py:152-154
            return self[np.random.randint(len(self))]
        return data


class _InfoFrames:
    """The frames of an infos list as database_sampler.create_groundtruth_database reads a dataset: len() and
    raw_sample(k) -> (points, the objects' LiDAR boxes, their names); DontCare entries carry no box."""

    def __init__(self, dataset, infos):
        self.dataset, self.infos = dataset, infos

    def __len__(self):
        return len(self.infos)

    def raw_sample(self, k):
        info = self.infos[k]
        boxes = np.asarray(info["annos"]["gt_boxes_lidar"], dtype=np.float32).reshape(-1, 7)
        return self.dataset.get_lidar(info["point_cloud"]["lidar_idx"]), boxes, info["annos"]["name"][:len(boxes)]


def create_kitti_infos(dataset_cfg, class_names, data_path, save_path, workers=4):
    """kitti_infos_{train,val,trainval,test}.pkl (a split without an ImageSets file is skipped) and the train split's GT database."""
    data_path, save_path = Path(data_path), Path(save_path)
    dataset = KittiDataset(dataset_cfg=dataset_cfg, class_names=class_names, root_path=data_path, training=False)
    infos = {}
    for split in ("train", "val", "test"):
        dataset.set_split(split)
        if dataset.sample_id_list is None:
            continue
        infos[split] = dataset.get_infos(num_workers=workers, has_label=split != "test", count_inside_pts=split != "test")
        with open(save_path / f"kitti_infos_{split}.pkl", "wb") as f:
            pickle.dump(infos[split], f)
        print(f"Kitti info {split} file is saved to {save_path / f'kitti_infos_{split}.pkl'}")
    if "train" in infos and "val" in infos:
        with open(save_path / "kitti_infos_trainval.pkl", "wb") as f:
            pickle.dump(infos["train"] + infos["val"], f)
    if "train" in infos:
        dataset.set_split("train")
        dataset.create_groundtruth_database(save_path / "kitti_infos_train.pkl", split="train")
    return infos


def main(argv=None):
    import argparse

    from ...config import AttrDict, cfg_from_yaml_file
    ap = argparse.ArgumentParser()
    ap.add_argument("command", choices=["create_kitti_infos"])
    ap.add_argument("cfg_file", help="dataset yaml, e.g. toda_amd/tools/cfgs/dataset_configs/kitti_dataset.yaml")
    ap.add_argument("--data_path", default=None, help="KITTI root; default: DATA_PATH of the yaml")
    args = ap.parse_args(argv)
    dataset_cfg = cfg_from_yaml_file(args.cfg_file, AttrDict())
    root = Path(args.data_path or dataset_cfg.DATA_PATH)
    create_kitti_infos(dataset_cfg, ["Car", "Pedestrian", "Cyclist"], data_path=root, save_path=root)


if __name__ == "__main__":
    main()
