"""NuScenesMixUpAdvDataset (behaviour of reference pcdet/datasets/nuscenes/nuscenes_mixup_adv_dataset.py): TODA stage 2 on
nuScenes frames read from disk - (adversarial, original) pairs of target-domain frames with intra-domain MixUp.

    gt_infos    INFO_PATH[mode]                        the labelled subset
    ps_infos    pseudo_info_path / PSEUDO_INFO_PATH    the pseudo-labelled subset as tools/generate_pseudo_labels --perturb writes
                                                       it: gt_boxes [k, 7] in the sensor frame (SHIFT_COOR undone), gt_names,
                                                       p_score, p_voxel_perturb [M, 3], p_voxel_coords [M, 3] (z, y, x)
    infos       gt_infos + ps_infos; len(self) = len(gt_infos) * REPEAT when REPEAT is set

Per item (reference :286-588): with probability 1 - MIXUP_PROB the same frame twice - a labelled frame (probability GT_PROB) or
a pseudo-labelled frame whose `adv` copy carries the adversarial edit; otherwise a MixUp with collision removal of two frames
drawn per MIXUP_TYPE (only_gt | ps_gt | gt_gt+ps | gt+ps_gt+ps; no_mixup: always a labelled frame twice), built once for `adv`
and once for `org`.  only_gt and ps_gt use names the reference never defines; they mean what
SyntheticMixupPairDataset.draw_mixup_indices makes of them.  Both halves then pass the DataAugmentor independently, their
transforms recorded for model_fn_decorator_cl, and the data processor (mixup_dataset.finish_half, which hands the augmentor the
boxes' names too: gt_sampling pastes into either half).  The objects of the GT database are cut from unshifted frames, so with
SHIFT_COOR their stored centres are moved once, at construction: a pasted box and its points then land in the shifted scene
(the reference pastes both at their unshifted height).

MI355X layout: a frame is always a CUDA tensor, also with MAX_SWEEPS 1 (SweepDataset.merge_info: one upload, one merge pass,
one compaction).  The adversarial edit (reference get_ps_adv_lidar_with_sweeps, :191-274) is ops.adv_edit
(csrc/adv_frame.hip): the host draws, per pseudo box above PSEUDO_THRESH and in box order, op = np.random.randint(3), frac = np.random.random() and a uint32 seed; the
frame's voxel keys are sorted once and uploaded with the gradients; the device finds the rows of every box, draws the subsets
and edits the cloud, which never returns to the host.  The reference's helper module (pcdet/utils/perturb_utils.py) is not
part of its tree: the voxel lookup and the box test are this project's, as in SyntheticMixupPairDataset.
adversarial_points_host is the same edit in numpy on the same draws: the test oracle and the bench baseline.

The sampling policy, the MixUp and the edit do not depend on the dataset: they live in mixup_dataset.MixUpAdvPairPolicy, which
KittiMixUpAdvDataset uses as well; this class adds the nuScenes frames, infos and boxes.

The subset of a box: the c - k rows with the smallest keys fmix32(seed ^ uint32(row * 0x9E3779B9)), k = min(floor(frac * c),
c - 1) - a uniformly random subset of the size the reference draws (k = randint(c), shuffle, [k:]), without the counts going to
the host first.

FILTER_MIN_POINTS_IN_GT applies to labelled frames (a pseudo info carries the num_lidar_pts of boxes it no longer has).  The
boxes keep 7 columns (PRED_VELOCITY False: pseudo boxes have no velocity), so SET_NAN_VELOCITY_TO_ZEROS finds nothing to do."""
import copy
import pickle
from pathlib import Path

import numpy as np

from ..augmentor.database_sampler import DataBaseSampler
# the pair policy and the edit are shared with KittiMixUpAdvDataset (mixup_dataset.MixUpAdvPairPolicy); the names below stay
# importable from this module
from ..mixup_dataset import (ADV_ADD, ADV_MODIFY, ADV_REMOVE, MIXUP_TYPES, MixUpAdvPairPolicy, _boxes7, draw_mixup_indices,  # noqa: F401
                             encode_frame, finish_half, fmix32, subset_keys, subset_size)
from .nuscenes_dataset import NuScenesDataset


class NuScenesMixUpAdvDataset(MixUpAdvPairPolicy, NuScenesDataset):
    def __init__(self, dataset_cfg, class_names, training=True, root_path=None, logger=None, pseudo_info_path=None):
        self.pseudo_info_path = pseudo_info_path if pseudo_info_path is not None else dataset_cfg.get("PSEUDO_INFO_PATH", None)
        if self.pseudo_info_path is None:
            raise ValueError("NuScenesMixUpAdvDataset needs pseudo_info_path (or DATA_CONFIG.PSEUDO_INFO_PATH): the infos file of "
                             "tools/generate_pseudo_labels --perturb")
        if dataset_cfg.get("PRED_VELOCITY", False):
            raise NotImplementedError("PRED_VELOCITY: pseudo boxes carry no velocity; NuScenesMixUpAdvDataset keeps 7 box columns")
        if dataset_cfg.get("BALANCED_RESAMPLING", False):
            raise NotImplementedError("BALANCED_RESAMPLING would mix the labelled and the pseudo-labelled infos the sampling policy tells apart")
        self.gt_infos, self.ps_infos = [], []
        super().__init__(dataset_cfg=dataset_cfg, class_names=class_names, training=training, root_path=root_path, logger=logger)
        self.on_device = True            # frames are CUDA tensors also with MAX_SWEEPS 1: build_dataloader keeps the dataset in the training process
        self.init_pair_policy(dataset_cfg, pseudo_thresh=0.3)
        if self.shift_coor and self.data_augmentor is not None:
            for step in self.data_augmentor.data_augmentor_queue:
                if isinstance(step, DataBaseSampler):
                    step.db_infos = {name: [self._shifted_object(i) for i in infos] for name, infos in step.db_infos.items()}

    def _shifted_object(self, info):
        """A GT-database record with SHIFT_COOR added to its box centre; the sampler puts the object's points around that centre."""
        box = np.array(info["box3d_lidar"], dtype=np.float32)
        box[0:3] += np.asarray(self.shift_coor, np.float32)
        return {**info, "box3d_lidar": box}

    # ---- reading
    def include_nuscenes_data(self, mode):
        super().include_nuscenes_data(mode)
        self.gt_infos = self.infos
        path = Path(self.pseudo_info_path)
        if not path.exists():
            raise FileNotFoundError(f"pseudo-label infos {path} do not exist: write them with tools/generate_pseudo_labels --perturb")
        with open(path, "rb") as f:
            self.ps_infos = list(pickle.load(f))
        self.infos = self.gt_infos + self.ps_infos
        self._log("GT samples for NuScenes dataset: %d, pseudo samples: %d" % (len(self.gt_infos), len(self.ps_infos)))

    def pseudo_frame(self, info, thres=None):
        """Drops the pseudo boxes with p_score < thres (reference :30-45); a labelled info passes."""
        if "p_score" in info:
            keep = ~(np.asarray(info["p_score"]) < (self.pseudo_thresh if thres is None else thres))
            info["gt_boxes"], info["gt_names"], info["p_score"] = info["gt_boxes"][keep], info["gt_names"][keep], info["p_score"][keep]
        return info

    def frame_points(self, info):
        """[n, 5] CUDA tensor of one info: key frame and MAX_SWEEPS - 1 sweeps merged, SHIFT_COOR added."""
        return self.merge_info(info, self.max_sweeps, shift=np.array(self.shift_coor, dtype=np.float32) if self.shift_coor else None)

    # ---- frames and items
    def frame(self, k, adversarial, draws=None):
        """Frame k of infos (labelled first, then pseudo-labelled) before prepare_data: {points (CUDA), gt_boxes [n, 7], gt_names,
        frame_id, metadata}; the `adversarial` copy of a pseudo-labelled frame carries the edit."""
        info = copy.deepcopy(self.infos[k])
        points = self.frame_points(info)
        if adversarial and not self.is_gt(k):
            points = self.adversarial_points(points, info, draws)
        info = self.pseudo_frame(info)
        min_points = self.dataset_cfg.get("FILTER_MIN_POINTS_IN_GT", False)
        keep = slice(None)
        if min_points and self.is_gt(k):
            keep = info["num_lidar_pts"] > min_points - 1
        boxes = _boxes7(info["gt_boxes"])[keep]
        if self.shift_coor:
            boxes[:, 0:3] += np.asarray(self.shift_coor, np.float32)
        return {"points": points, "gt_boxes": boxes, "gt_names": np.asarray(info["gt_names"])[keep], "frame_id": Path(info["lidar_path"]).stem,
                "metadata": {"token": info["token"]}}
