"""DataAugmentor (reference pcdet/datasets/augmentor/data_augmentor.py:9-257): a queue of augmentations selected by NAME
from DATA_AUGMENTOR.AUG_CONFIG_LIST.  Built: gt_sampling (database_sampler.py), random_world_flip / random_world_rotation /
random_world_scaling / random_world_translation, random_local_translation / _rotation / _scaling, random_world_ /
random_local_frustum_dropout and random_local_pyramid_aug - all on the device for CUDA clouds.  The applied transforms are
recorded in data_dict['augmentation_list' / 'augmentation_params'] - the stage-2 consistency step undoes them on the
decoded boxes (models.reverse_transform)."""
from functools import partial

import numpy as np

from ...utils import common_utils
from . import augmentor_utils


class DataAugmentor:
    def __init__(self, root_path, augmentor_configs, class_names, logger=None):
        self.root_path, self.class_names, self.logger = root_path, class_names, logger
        cfgs = augmentor_configs if isinstance(augmentor_configs, list) else augmentor_configs.AUG_CONFIG_LIST
        disabled = [] if isinstance(augmentor_configs, list) else list(augmentor_configs.get("DISABLE_AUG_LIST", []))
        self.data_augmentor_queue = [getattr(self, c.NAME)(config=c) for c in cfgs if c.NAME not in disabled]

    def gt_sampling(self, config=None):
        from .database_sampler import DataBaseSampler
        return DataBaseSampler(root_path=self.root_path, sampler_cfg=config, class_names=self.class_names, logger=self.logger)

    @staticmethod
    def _record(data_dict, name, value):
        data_dict.setdefault("augmentation_list", []).append(name)
        data_dict.setdefault("augmentation_params", {})[name] = value

    def random_world_flip(self, data_dict=None, config=None):
        if data_dict is None:
            return partial(self.random_world_flip, config=config)
        gt_boxes, points = data_dict["gt_boxes"], data_dict["points"]
        flipped = []
        for axis in config["ALONG_AXIS_LIST"]:
            assert axis in ("x", "y")
            gt_boxes, points, on = getattr(augmentor_utils, f"random_flip_along_{axis}")(gt_boxes, points, return_flip=True)
            if on:
                flipped.append(axis)
        data_dict["gt_boxes"], data_dict["points"] = gt_boxes, points
        self._record(data_dict, "random_world_flip", flipped)
        return data_dict

    def random_world_rotation(self, data_dict=None, config=None):
        if data_dict is None:
            return partial(self.random_world_rotation, config=config)
        rot_range = config["WORLD_ROT_ANGLE"]
        if not isinstance(rot_range, list):
            rot_range = [-rot_range, rot_range]
        data_dict["gt_boxes"], data_dict["points"], angle = augmentor_utils.global_rotation(
            data_dict["gt_boxes"], data_dict["points"], rot_range=rot_range, return_rot=True)
        self._record(data_dict, "random_world_rotation", angle)
        return data_dict

    def random_world_scaling(self, data_dict=None, config=None):
        if data_dict is None:
            return partial(self.random_world_scaling, config=config)
        data_dict["gt_boxes"], data_dict["points"], scale = augmentor_utils.global_scaling(
            data_dict["gt_boxes"], data_dict["points"], config["WORLD_SCALE_RANGE"], return_scale=True)
        self._record(data_dict, "random_world_scaling", scale)
        return data_dict

    # ---- per-object and pyramid augmentations (reference :101-226).  Not recorded in augmentation_list: the stage-2
    # reverse_transform undoes world flips, rotations and scalings only, as in the reference.
    @staticmethod
    def _axis_chain(data_dict, axes, arg, host_name, build):
        """The translation family: one function call per axis on numpy clouds; on CUDA clouds the step tables of all
        axes (they depend on the boxes alone) are joined and run in one launch."""
        gt_boxes, points = data_dict["gt_boxes"], data_dict["points"]
        for axis in axes:
            assert axis in ("x", "y", "z")
        if augmentor_utils._on_device(points):
            tables = [build(gt_boxes, arg, axis) for axis in axes]
            points = augmentor_utils._run_steps(points, np.concatenate(tables, axis=0)) if tables else points
        else:
            for axis in axes:
                gt_boxes, points = getattr(augmentor_utils, host_name % axis)(gt_boxes, points, arg)
        data_dict["gt_boxes"], data_dict["points"] = gt_boxes, points
        return data_dict

    def random_world_translation(self, data_dict=None, config=None):
        if data_dict is None:
            return partial(self.random_world_translation, config=config)
        if config["NOISE_TRANSLATE_STD"] == 0:
            return data_dict
        return self._axis_chain(data_dict, config["ALONG_AXIS_LIST"], config["NOISE_TRANSLATE_STD"], "random_translation_along_%s",
                                augmentor_utils.world_translation_steps)

    def random_local_translation(self, data_dict=None, config=None):
        if data_dict is None:
            return partial(self.random_local_translation, config=config)
        return self._axis_chain(data_dict, config["ALONG_AXIS_LIST"], config["LOCAL_TRANSLATION_RANGE"],
                                "random_local_translation_along_%s", augmentor_utils.local_translation_steps)

    def random_local_rotation(self, data_dict=None, config=None):
        if data_dict is None:
            return partial(self.random_local_rotation, config=config)
        rot_range = config["LOCAL_ROT_ANGLE"]
        if not isinstance(rot_range, list):
            rot_range = [-rot_range, rot_range]
        data_dict["gt_boxes"], data_dict["points"] = augmentor_utils.local_rotation(data_dict["gt_boxes"], data_dict["points"], rot_range=rot_range)
        return data_dict

    def random_local_scaling(self, data_dict=None, config=None):
        if data_dict is None:
            return partial(self.random_local_scaling, config=config)
        data_dict["gt_boxes"], data_dict["points"] = augmentor_utils.local_scaling(data_dict["gt_boxes"], data_dict["points"], config["LOCAL_SCALE_RANGE"])
        return data_dict

    def random_world_frustum_dropout(self, data_dict=None, config=None):
        """Boxes beyond the threshold leave with the points; their names (and the class mask of forward()) follow, which the
        reference leaves out of step."""
        if data_dict is None:
            return partial(self.random_world_frustum_dropout, config=config)
        gt_boxes, points = data_dict["gt_boxes"], data_dict["points"]
        for direction in config["DIRECTION"]:
            assert direction in ("top", "bottom", "left", "right")
            gt_boxes, points, keep = getattr(augmentor_utils, f"global_frustum_dropout_{direction}")(
                gt_boxes, points, config["INTENSITY_RANGE"], return_mask=True)
            for key in ("gt_names", "gt_boxes_mask"):
                if key in data_dict:
                    data_dict[key] = data_dict[key][keep]
        data_dict["gt_boxes"], data_dict["points"] = gt_boxes, points
        return data_dict

    def random_local_frustum_dropout(self, data_dict=None, config=None):
        if data_dict is None:
            return partial(self.random_local_frustum_dropout, config=config)
        gt_boxes, points = data_dict["gt_boxes"], data_dict["points"]
        for direction in config["DIRECTION"]:
            assert direction in ("top", "bottom", "left", "right")
            gt_boxes, points = getattr(augmentor_utils, f"local_frustum_dropout_{direction}")(gt_boxes, points, config["INTENSITY_RANGE"])
        data_dict["gt_boxes"], data_dict["points"] = gt_boxes, points
        return data_dict

    def random_local_pyramid_aug(self, data_dict=None, config=None):
        """SE-SSD's shape-aware augmentation: pyramid dropout, then sparsify, then swap, each on the boxes the last left."""
        if data_dict is None:
            return partial(self.random_local_pyramid_aug, config=config)
        gt_boxes, points = data_dict["gt_boxes"], data_dict["points"]
        gt_boxes, points, pyramids = augmentor_utils.local_pyramid_dropout(gt_boxes, points, config["DROP_PROB"])
        gt_boxes, points, pyramids = augmentor_utils.local_pyramid_sparsify(gt_boxes, points, config["SPARSIFY_PROB"],
                                                                            config["SPARSIFY_MAX_NUM"], pyramids)
        gt_boxes, points = augmentor_utils.local_pyramid_swap(gt_boxes, points, config["SWAP_PROB"], config["SWAP_MAX_NUM"], pyramids)
        data_dict["gt_boxes"], data_dict["points"] = gt_boxes, points
        return data_dict

    def forward(self, data_dict):
        for step in self.data_augmentor_queue:
            data_dict = step(data_dict=data_dict)
        data_dict["gt_boxes"][:, 6] = common_utils.limit_period(data_dict["gt_boxes"][:, 6], offset=0.5, period=2 * np.pi)
        data_dict.pop("calib", None)
        data_dict.pop("road_plane", None)
        if "gt_boxes_mask" in data_dict:
            keep = data_dict.pop("gt_boxes_mask")
            data_dict["gt_boxes"] = data_dict["gt_boxes"][keep]
            data_dict["gt_names"] = data_dict["gt_names"][keep]
        return data_dict
