"""KittiMixUpAdvDataset (behaviour of reference pcdet/datasets/kitti/kitti_mixup_adv_dataset.py): TODA stage 2 on KITTI frames
read from disk - (adversarial, original) pairs of target-domain frames with intra-domain MixUp, for the nuScenes -> KITTI arm
with SECOND-IoU.

    infos       INFO_PATH[mode]: every training frame, with annotations
    split file  LABELLED_SPLIT_FILE (default ImageSets/<split>_0.01_1.txt): lines `<frame id> <index into infos>`, the labelled
                subset; each id is checked against the info's point_cloud.lidar_idx
    pseudo      pseudo_info_path / PSEUDO_INFO_PATH, as tools/generate_pseudo_labels --perturb writes it from
                KittiDataset.dump_infos: the same frames in the same order, with gt_boxes [k, 7] in the sensor frame (SHIFT_COOR
                undone), gt_names, p_score, p_voxel_perturb [M, 3], p_voxel_coords [M, 3] (z, y, x)
    gt_infos    the infos at the listed indices
    ps_infos    the pseudo infos at all other indices; when the list covers every info, the pseudo infos at the listed indices
                (the reference tells "everything" by the constant 3712, the size of KITTI's train split)

The sampling policy, the MixUp and the adversarial edit are mixup_dataset.MixUpAdvPairPolicy's, shared with
NuScenesMixUpAdvDataset.  The edit visits the boxes with p_score > PSEUDO_THRESH (default 0.2, reference get_adv_points) and
moves x, y, z of the [n, 4] rows (ops.adv_edit at c = 4); the training boxes of a pseudo-labelled frame are all boxes of its
info - they were thresholded when the infos were written.  A labelled frame takes its boxes from `annos` (camera -> LiDAR,
DontCare dropped).  Both are shifted by SHIFT_COOR.

MI355X layout: a frame is read once, cropped to the camera's field of view on the device (ops.points_fov_flags,
csrc/kitti_frame.hip) and shifted; inside one item the `adv` and the `org` copy of a frame share that read and that crop (the
reference reads the file two to four times per item).

gt_sampling stays disabled, as in the reference's nuScenes -> KITTI configuration: pasting KITTI objects needs the road planes
of both halves; enabling it is an error at construction.  Evaluation is KittiDataset's, on the full infos."""
import copy
import pickle
from pathlib import Path

import numpy as np
import torch

from ...utils import box_utils, common_utils
from ..mixup_dataset import MixUpAdvPairPolicy, _boxes7
from .kitti_dataset import KittiDataset


def read_labelled_split(listing, infos):
    """The indices of a labelled split file, lines of `<frame id> <index into the infos>`, in the file's order; raises when a
    listed id does not sit at its index (tools/make_labelled_subset.py writes such files)."""
    listed = []
    for line in open(listing).read().splitlines():
        if not line.strip():
            continue
        frame, index = line.split()[0], int(line.split()[1])
        if not 0 <= index < len(infos) or str(infos[index]["point_cloud"]["lidar_idx"]) != frame:
            have = infos[index]["point_cloud"]["lidar_idx"] if 0 <= index < len(infos) else "no such info"
            raise ValueError(f"{listing}: line `{line.strip()}` names frame {frame} at index {index}, the infos hold {have} there")
        listed.append(index)
    return listed


class KittiMixUpAdvDataset(MixUpAdvPairPolicy, KittiDataset):
    def __init__(self, dataset_cfg, class_names, training=True, root_path=None, logger=None, pseudo_info_path=None):
        self.pseudo_info_path = pseudo_info_path if pseudo_info_path is not None else dataset_cfg.get("PSEUDO_INFO_PATH", None)
        if self.pseudo_info_path is None:
            raise ValueError("KittiMixUpAdvDataset needs pseudo_info_path (or DATA_CONFIG.PSEUDO_INFO_PATH): the infos file of "
                             "tools/generate_pseudo_labels --perturb")
        aug = dataset_cfg.get("DATA_AUGMENTOR", None)
        if training and aug is not None:
            disabled = list(aug.get("DISABLE_AUG_LIST", []))
            if any(c.NAME == "gt_sampling" and c.NAME not in disabled for c in aug.AUG_CONFIG_LIST):
                raise NotImplementedError("gt_sampling in KittiMixUpAdvDataset: pasting needs the road planes of both halves of a pair, which is "
                                          "not built; keep it in DATA_AUGMENTOR.DISABLE_AUG_LIST")
        self.gt_infos, self.ps_infos, self.infos = [], [], []
        self._crops = None
        super().__init__(dataset_cfg=dataset_cfg, class_names=class_names, training=training, root_path=root_path, logger=logger)
        self.on_device = True            # frames are CUDA tensors: build_dataloader keeps the dataset in the training process
        self.init_pair_policy(dataset_cfg, pseudo_thresh=0.2)

    # ---- reading
    def include_kitti_data(self, mode):
        super().include_kitti_data(mode)
        infos = self.kitti_infos
        rel = self.dataset_cfg.get("LABELLED_SPLIT_FILE", None) or f"ImageSets/{self.split}_0.01_1.txt"
        listing = self.root_path / rel
        if not listing.exists():
            raise FileNotFoundError(f"labelled split file {listing} does not exist: lines of `<frame id> <index into the infos>`")
        listed = read_labelled_split(listing, infos)
        path = Path(self.pseudo_info_path)
        if not path.exists():
            raise FileNotFoundError(f"pseudo-label infos {path} do not exist: write them with tools/generate_pseudo_labels --perturb")
        with open(path, "rb") as f:
            pseudo = list(pickle.load(f))
        ids = [str(i["point_cloud"]["lidar_idx"]) for i in infos]
        if len(pseudo) != len(infos) or [str(p["point_cloud"]["lidar_idx"]) for p in pseudo] != ids:
            raise ValueError(f"pseudo-label infos {path}: {len(pseudo)} frames that are not the {len(infos)} frames of INFO_PATH in their "
                             "order; write them from this dataset's own infos (KittiDataset.dump_infos)")
        chosen = set(listed)
        others = [k for k in range(len(infos)) if k not in chosen]
        self.gt_infos = [infos[k] for k in listed]
        self.ps_infos = [pseudo[k] for k in (others if others else listed)]
        self.infos = self.gt_infos + self.ps_infos
        if self.logger is not None:
            self.logger.info("GT samples for KITTI dataset: %d, pseudo samples: %d" % (len(self.gt_infos), len(self.ps_infos)))

    # ---- frames
    def frame_points(self, info):
        """[n, 4] CUDA tensor of one info: the rows inside the camera image (FOV_POINTS_ONLY), SHIFT_COOR added.  Inside raw_pair
        a frame is read and cropped once, every user gets a copy of it."""
        idx = info["point_cloud"]["lidar_idx"]
        if self._crops is not None and idx in self._crops:
            return self._crops[idx].clone()
        points = self.get_lidar(idx)
        if self.fov_points_only:
            points = self.fov_points(points, self.get_calib(idx), info["image"]["image_shape"])
        else:
            points = torch.from_numpy(np.ascontiguousarray(points, dtype=np.float32)).cuda()
        if self.shift_coor:
            points = points + torch.from_numpy(np.array(list(self.shift_coor) + [0.0] * (points.shape[1] - 3), dtype=np.float32)).to(points.device)
        if self._crops is not None:
            self._crops[idx] = points
            return points.clone()
        return points

    def frame_boxes(self, info):
        """(boxes [k, 7] fp32 with SHIFT_COOR added, names): a labelled info's annotations (camera -> LiDAR, DontCare dropped), a
        pseudo info's gt_boxes - all of them."""
        if "annos" in info and "gt_boxes" not in info:
            annos = common_utils.drop_info_with_name(copy.deepcopy(info["annos"]), name="DontCare")
            cam = np.concatenate([annos["location"], annos["dimensions"], annos["rotation_y"][..., np.newaxis]], axis=1).astype(np.float32)
            boxes = box_utils.boxes3d_kitti_camera_to_lidar(cam, self.get_calib(info["point_cloud"]["lidar_idx"])).astype(np.float32)
            boxes, names = boxes.reshape(-1, 7), np.asarray(annos["name"])
        else:
            boxes, names = _boxes7(info["gt_boxes"]), np.asarray(info["gt_names"])
        if self.shift_coor:
            boxes[:, 0:3] += np.asarray(self.shift_coor, np.float32)
        return boxes, names

    def frame(self, k, adversarial, draws=None):
        """Frame k of infos (labelled first, then pseudo-labelled) before prepare_data: {points (CUDA), gt_boxes [n, 7], gt_names,
        frame_id}; the `adversarial` copy of a pseudo-labelled frame carries the edit."""
        info = self.infos[k]
        points = self.frame_points(info)
        if adversarial and not self.is_gt(k):
            points = self.adversarial_points(points, info, draws)
        boxes, names = self.frame_boxes(info)
        return {"points": points, "gt_boxes": boxes, "gt_names": names, "frame_id": info["point_cloud"]["lidar_idx"]}

    def raw_pair(self, item):
        self._crops = {}
        try:
            return super().raw_pair(item)
        finally:
            self._crops = None
