"""Two-domain mixing dataset of TODA stage 1 (reference pcdet/datasets/two_dataset.py:164-290 `prepare_data` and the
sampling policy of pcdet/datasets/mix_dataset/waymo_nus_{polarmix,cutmix,lasermix}_dataset.py:154-320).

MI355X layout: both raw clouds are uploaded once and stay in HBM; feature encoding, the mix
(processor/point_mix.py), the range mask and the shuffle all run on the device and the sample leaves
`__getitem__` as a CUDA tensor that `voxelize_on_gpu` consumes - nothing of the cloud returns to the host.
Use with num_workers = 0 (the training process owns the GPU).

Config keys (as in the reference YAMLs, e.g. tools/cfgs/stage1_targetmix/*.yaml):
  MIX_TYPE: polarmix | cutmix | cutpolarmix | lasermix | pseudobbox | pseudobackground     MIX_INC_METHOD: center | corner | corner_del
  POLARMIX_PROB (CUTMIX_PROB for cutmix; the LaserMix and pseudo-mix datasets of the reference read POLARMIX_PROB too,
  waymo_nus_lasermix_dataset.py:153) = probability of a mixed sample, POLARMIX_DEGREE, POLARMIX_RC_NUM, POLARMIX_UPDATE_METHOD,
  POLARMIX_DIS (FULL | RAND), POLARMIX_USE_PITCH, LASERMIX_NUM_AREAS, LASERMIX_NUM_ANGLES (absent: the spherical variant,
  tools/cfgs/stage1_lasermix/*_pp01.yaml), LASERMIX_PITCH_ANGLE
  SYNTHETIC: {SOURCE_KIND, TARGET_KIND, NUM_SOURCE, NUM_TARGET, SEED}   (SyntheticMixDataset: no real dataset on the box)
  WaymoDataset: {...}, NuScenesDataset: {...}                             (WaymoNusMixDataset: the two domains' own dataset
  configs, each with CLASS_NAMES and DATA_AUGMENTOR, as the reference's stage-1 YAMLs write them)
  NuScenesDataset: {...}, KittiDataset: {...}                             (NusKittiMixDataset, likewise)

TwoDomainMixDataset holds what the real two-domain datasets share: the length, the index policy, both redraws and the
preparation of one domain's frame.  WaymoNusMixDataset (WaymoNusPolarMixDataset / ...CutMix... / ...LaserMix...) takes source
frames from a WaymoDataset and target frames from a NuScenesDataset; NusKittiMixDataset (NusKittiPolarMixDataset /
...CutMix...) takes source frames from a NuScenesDataset and target frames from a KittiDataset.  Each is one class under the
reference's several names: MIX_TYPE decides the mix.  The trained model is evaluated through the DATA_CONFIG_TEST block of the
same YAML (tools/test.py), the labelled-subset files the YAMLs name come from tools/make_labelled_subset.py.  Of the stage-2
real mixup datasets, NuScenesMixUpAdvDataset (nuscenes/nuscenes_mixup_adv_dataset.py) and KittiMixUpAdvDataset
(kitti/kitti_mixup_adv_dataset.py) are built; the non-adversarial NuScenesMixUpDataset is not.
"""
import numpy as np
import torch

from ..config import AttrDict
from .dataset import DatasetTemplate
from .processor.inter_domain_point_cutmix import inter_domain_point_cutmix
from .processor.inter_domain_point_lasermix import inter_domain_point_lasermix
from .processor.inter_domain_point_polarmix import inter_domain_point_polarmix
from .processor.inter_domain_point_pseudomix import inter_domain_point_pseudobackground, inter_domain_point_pseudobbox
from .synthetic import synth_cloud


class MixDatasetTemplate(DatasetTemplate):
    """What the two-domain datasets share: the mix settings of the config and the MIX_TYPE switch."""

    def __init__(self, dataset_cfg, class_names, training=True, root_path=None, logger=None):
        super().__init__(dataset_cfg=dataset_cfg, class_names=class_names, training=training, root_path=root_path, logger=logger)
        self.mix_type = dataset_cfg.get("MIX_TYPE", "polarmix")
        if self.mix_type not in ("polarmix", "cutmix", "cutpolarmix", "lasermix", "pseudobbox", "pseudobackground"):
            raise NotImplementedError(self.mix_type)
        prob_key = "CUTMIX_PROB" if self.mix_type == "cutmix" else "POLARMIX_PROB"
        if self.mix_type == "lasermix" and "LASERMIX_PROB" in dataset_cfg:       # this repo's earlier spelling
            prob_key = "LASERMIX_PROB"
        self.mix_prob = float(dataset_cfg.get(prob_key, 0.5))
        self.mix_inc_method = dataset_cfg.get("MIX_INC_METHOD", "center")
        self.polarmix_rot_copy_num = int(dataset_cfg.get("POLARMIX_RC_NUM", 1))
        self.polarmix_degree = dataset_cfg.get("POLARMIX_DEGREE", 1.570796)
        self.polarmix_update_method = list(dataset_cfg.get("POLARMIX_UPDATE_METHOD", ["FIX", "FIX", "FIX"]))
        self.polarmix_dis = dataset_cfg.get("POLARMIX_DIS", "FULL")
        self.polarmix_use_pitch = bool(dataset_cfg.get("POLARMIX_USE_PITCH", False))
        # defaults of waymo_nus_lasermix_dataset.py:34-36 (no LASERMIX_NUM_ANGLES: the spherical variant)
        self.laser_pitch_angle = dataset_cfg.get("LASERMIX_PITCH_ANGLE", [-20, 0])
        self.laser_num_areas = dataset_cfg.get("LASERMIX_NUM_AREAS", 3)
        self.laser_num_angles = dataset_cfg.get("LASERMIX_NUM_ANGLES", None)
        self.train_percent = 0.0          # the trainer moves it from 0 to 1 (reference train_utils: cur_it / total_it)

    def set_train_percent(self, value):
        self.train_percent = float(value)

    def mix(self, source, target):
        """The MIX_TYPE switch of the reference's prepare_data (two_dataset.py:227-268)."""
        kind = self.mix_type
        if kind == "cutpolarmix":
            kind = "cutmix" if np.random.random() < 0.5 else "polarmix"
        if kind == "cutmix":
            return inter_domain_point_cutmix(source, target, self.point_cloud_range, self.mix_inc_method)
        if kind == "polarmix":
            return inter_domain_point_polarmix(source, target, self.polarmix_rot_copy_num, self.polarmix_degree, self.train_percent,
                                               self.polarmix_update_method, self.point_cloud_range, self.polarmix_dis,
                                               self.mix_inc_method, self.polarmix_use_pitch)
        if kind == "lasermix":
            return inter_domain_point_lasermix(source, target, self.laser_pitch_angle, self.laser_num_areas, self.laser_num_angles,
                                               self.point_cloud_range, self.mix_inc_method)
        if kind == "pseudobbox":
            return inter_domain_point_pseudobbox(source, target)
        if kind == "pseudobackground":
            return inter_domain_point_pseudobackground(source, target)
        raise NotImplementedError(kind)


class SyntheticMixDataset(MixDatasetTemplate):
    def __init__(self, dataset_cfg, class_names, training=True, root_path=None, logger=None):
        super().__init__(dataset_cfg=dataset_cfg, class_names=class_names, training=training, root_path=root_path, logger=logger)
        syn = dataset_cfg.get("SYNTHETIC", AttrDict())
        self.source_kind, self.target_kind = syn.get("SOURCE_KIND", "waymo_toda"), syn.get("TARGET_KIND", "nuscenes_toda")
        self.num_source, self.num_target = int(syn.get("NUM_SOURCE", 32)), int(syn.get("NUM_TARGET", 32))
        self.seed = int(syn.get("SEED", 0))
        self.num_points = {self.source_kind: syn.get("NUM_POINTS_SOURCE", None), self.target_kind: syn.get("NUM_POINTS_TARGET", None)}
        self.on_device = bool(dataset_cfg.get("MIX_ON_DEVICE", True))
        # keep generated frames: True = resident on the device, "host" = points in pinned host memory, uploaded at every access
        self.cache_frames = dataset_cfg.get("CACHE_FRAMES", False)
        self._cache = {}

    def __len__(self):
        return self.num_source + self.num_target

    # ---- one domain's frame: raw points (+ upload), boxes with the class-id column, encoded features
    def _frame(self, kind, index):
        host = self.cache_frames == "host" and self.on_device
        if self.cache_frames and (kind, index) in self._cache:
            data = dict(self._cache[(kind, index)])
            if host:
                data["points"] = data["points"].cuda(non_blocking=True)      # on the caller's current stream
            return data
        data = self._make_frame(kind, index)
        if self.cache_frames:
            kept = dict(data)
            if host:
                kept["points"] = data["points"].cpu().pin_memory()
            self._cache[(kind, index)] = kept
        return data

    def _make_frame(self, kind, index):
        n_points = self.num_points.get(kind)
        points, boxes, names = synth_cloud(kind, self.seed + index, n_points, class_count=len(self.class_names))
        names = np.array([self.class_names[int(n[3:]) - 1] for n in names])
        points = points[:, :len(self.point_feature_encoder.src_feature_list)]
        keep = np.array([n in self.class_names for n in names], dtype=bool)
        ids = np.array([self.class_names.index(n) + 1 for n in names[keep]], dtype=np.float32).reshape(-1, 1)
        data = {"points": torch.from_numpy(points).cuda() if self.on_device else points,
                "gt_boxes": np.concatenate([boxes[keep], ids], axis=1).astype(np.float32), "frame_id": f"{kind}_{index:06d}"}
        return self.point_feature_encoder.forward(data)

    def __getitem__(self, index):
        if np.random.random(1) < self.mix_prob:
            source = self._frame(self.source_kind, index % self.num_source)
            target = self._frame(self.target_kind, 100_000 + index % self.num_target)
            data = self.mix(source, target)
            if data["gt_boxes"].ndim != 2:                               # reference :271-273: draw another sample
                return self[np.random.randint(len(self))]
            data["frame_id"] = f"mix_{index:06d}"
        elif index < self.num_source:
            data = self._frame(self.source_kind, index)
        else:
            data = self._frame(self.target_kind, 100_000 + index - self.num_source)
        data = self.data_processor.forward(data)
        if self.training and len(data["gt_boxes"]) == 0:
            return self[np.random.randint(len(self))]
        return data


class TwoDomainMixDataset(MixDatasetTemplate):
    """The real two-domain dataset of stage 1: `self.source` and `self.target` are two datasets read from disk, each built from
    its sub-block of DATA_CONFIG (own DATA_PATH, CLASS_NAMES and DATA_AUGMENTOR); the joint POINT_FEATURE_ENCODING and
    DATA_PROCESSOR apply to both domains.  A subclass builds the two datasets and gives the two hooks source_frame(i) and
    target_frame(i), each a domain's raw frame through _prepare_domain; the length, the index policy and both redraws are here
    (reference mix_dataset/*_dataset.py + two_dataset.py:100-296)."""
    on_device = True

    @property
    def num_source(self):
        return len(self.source.infos)

    @property
    def num_target(self):
        return len(self.target.infos)

    def __len__(self):
        if self._merge_all_iters_to_one_epoch:
            return (self.num_source + self.num_target) * self.total_epochs
        return self.num_source + self.num_target

    def source_frame(self, index):
        raise NotImplementedError

    def target_frame(self, index):
        raise NotImplementedError

    # ---- one domain's frame as the mix takes it: augmented by the domain's own augmentor, boxes [n, 7] + the class id of the
    # domain's own list, the domain's first class under the joint first name, features encoded by the joint encoder.  A frame
    # without an object of the domain's classes leaves with [0, 8] boxes and an empty string array of names.
    def _prepare_domain(self, domain, data):
        names_of = domain.class_names
        if self.training:
            assert "gt_boxes" in data, "gt_boxes should be provided for training"
            if domain.data_augmentor is not None:
                mask = np.array([n in names_of for n in data["gt_names"]], dtype=bool)
                data = domain.data_augmentor.forward({**data, "gt_boxes_mask": mask})
        if data.get("gt_boxes") is not None:
            names = data["gt_names"]
            keep = np.array([n in names_of for n in names], dtype=bool)
            ids = np.array([names_of.index(n) + 1 for n in names[keep]], dtype=np.float32).reshape(-1, 1)
            data["gt_boxes"] = np.concatenate([data["gt_boxes"][keep], ids], axis=1).astype(np.float32)
            data["gt_names"] = np.array([self.class_names[0] if n == names_of[0] else n for n in names[keep]], dtype=str)
        if not torch.is_tensor(data["points"]):                     # MAX_SWEEPS 1: the key frame came from the host route
            data["points"] = torch.from_numpy(np.ascontiguousarray(data["points"], dtype=np.float32))
        data["points"] = data["points"].cuda()
        return self.point_feature_encoder.forward(data)

    def __getitem__(self, index):
        if self._merge_all_iters_to_one_epoch:
            index = index % (self.num_source + self.num_target)     # the reference multiplies here, which leaves the range
        if np.random.random(1) < self.mix_prob:
            source = self.source_frame(index % self.num_source)
            target = self.target_frame(index % self.num_target)
            data = self.mix(source, target)
            if data["gt_boxes"].ndim != 2:                               # reference two_dataset.py:271-273: draw another sample
                return self[np.random.randint(len(self))]
        elif index < self.num_source:
            data = self.source_frame(index)
        else:
            data = self.target_frame(index - self.num_source)
        data = self.data_processor.forward(data)
        if self.training and len(data["gt_boxes"]) == 0:
            return self[np.random.randint(len(self))]
        data.pop("gt_names", None)
        return data


def _nuscenes_mix_frame(domain, index):
    """A NuScenesDataset's raw frame as a mix takes it: shift_coor noted, NaN velocities zeroed, boxes cut to 7 columns (the
    joint head has no velocity target)."""
    data = domain.raw_frame(index)
    cfg = domain.dataset_cfg
    if "gt_boxes" in data:
        if cfg.get("SHIFT_COOR", None):
            data["shift_coor"] = cfg.SHIFT_COOR
        if cfg.get("SET_NAN_VELOCITY_TO_ZEROS", False):
            data["gt_boxes"][np.isnan(data["gt_boxes"])] = 0
        data["gt_boxes"] = data["gt_boxes"][:, 0:7]
    return data


class WaymoNusMixDataset(TwoDomainMixDataset):
    """Waymo -> nuScenes: source frames from a WaymoDataset, target frames from a NuScenesDataset (reference
    mix_dataset/waymo_nus_*_dataset.py)."""

    def __init__(self, dataset_cfg, class_names, training=True, root_path=None, logger=None):
        from .nuscenes.nuscenes_dataset import NuScenesDataset
        from .waymo.waymo_dataset import WaymoDataset
        super().__init__(dataset_cfg=dataset_cfg, class_names=class_names, training=training, root_path=None, logger=logger)
        src_cfg, tgt_cfg = dataset_cfg["WaymoDataset"], dataset_cfg["NuScenesDataset"]
        self.source = WaymoDataset(src_cfg, src_cfg.CLASS_NAMES, training=training, logger=logger)
        self.target = NuScenesDataset(tgt_cfg, tgt_cfg.CLASS_NAMES, training=training, logger=logger)

    def source_frame(self, index):
        data = self.source.raw_frame(index)
        data.pop("num_points_in_gt", None)
        if "gt_boxes" in data:
            data["gt_boxes"] = data["gt_boxes"][:, 0:7]
        return self._prepare_domain(self.source, data)

    def target_frame(self, index):
        return self._prepare_domain(self.target, _nuscenes_mix_frame(self.target, index))


class NusKittiMixDataset(TwoDomainMixDataset):
    """nuScenes -> KITTI: source frames from a NuScenesDataset, target frames from a KittiDataset whose points reach the device
    in raw_frame (reference mix_dataset/nus_kitti_{polarmix,cutmix}_dataset.py:135-334).  A KITTI row has 4 columns where the
    joint src_feature_list names 5: the encoder only looks up `intensity`, column 3 in both.  Many KITTI frames hold no object
    of the target classes; such a frame still mixes (source boxes only) and, alone, is redrawn in training.

    Deviations from the reference:
      * KittiDataset.FOV_POINTS_ONLY: True is honoured in both branches, with the device crop; the reference raises NameError
        there (`points` is undefined, nus_kitti_polarmix_dataset.py:216-219), which is why its YAML sets False.
      * GET_ITEM_LIST is read from the KittiDataset sub-block in both branches; the reference reads the top level in the mixed
        branch and the sub-block in the other.
      * The merged-epochs index is a modulo, as in WaymoNusMixDataset; the reference multiplies."""

    def __init__(self, dataset_cfg, class_names, training=True, root_path=None, logger=None):
        from .kitti.kitti_dataset import KittiDataset
        from .nuscenes.nuscenes_dataset import NuScenesDataset
        super().__init__(dataset_cfg=dataset_cfg, class_names=class_names, training=training, root_path=None, logger=logger)
        src_cfg, tgt_cfg = dataset_cfg["NuScenesDataset"], dataset_cfg["KittiDataset"]
        self.source = NuScenesDataset(src_cfg, src_cfg.CLASS_NAMES, training=training, logger=logger)
        self.target = KittiDataset(tgt_cfg, tgt_cfg.CLASS_NAMES, training=training, logger=logger)

    @property
    def num_target(self):
        return len(self.target.kitti_infos)

    def source_frame(self, index):
        return self._prepare_domain(self.source, _nuscenes_mix_frame(self.source, index))

    def target_frame(self, index):
        return self._prepare_domain(self.target, self.target.raw_frame(index, device=True))       # the boxes have 7 columns
