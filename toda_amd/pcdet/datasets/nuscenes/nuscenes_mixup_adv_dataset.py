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

MI355X layout: a frame is always a CUDA tensor, also with MAX_SWEEPS 1 (one upload, ops.sweeps_merge, one compaction).  The
adversarial edit (reference get_ps_adv_lidar_with_sweeps, :191-274) is ops.adv_edit (csrc/adv_frame.hip): the host draws, per
pseudo box above PSEUDO_THRESH and in box order, op = np.random.randint(3), frac = np.random.random() and a uint32 seed; the
frame's voxel keys are sorted once and uploaded with the gradients; the device finds the rows of every box, draws the subsets
and edits the cloud, which never returns to the host.  The reference's helper module (pcdet/utils/perturb_utils.py) is not
part of its tree: the voxel lookup and the box test are this project's, as in SyntheticMixupPairDataset.
adversarial_points_host is the same edit in numpy on the same draws: the test oracle and the bench baseline.

The subset of a box: the c - k rows with the smallest keys fmix32(seed ^ uint32(row * 0x9E3779B9)), k = min(floor(frac * c),
c - 1) - a uniformly random subset of the size the reference draws (k = randint(c), shuffle, [k:]), without the counts going to
the host first.

FILTER_MIN_POINTS_IN_GT applies to labelled frames (a pseudo info carries the num_lidar_pts of boxes it no longer has).  The
boxes keep 7 columns (PRED_VELOCITY False: pseudo boxes have no velocity), so SET_NAN_VELOCITY_TO_ZEROS finds nothing to do."""
import copy
import pickle
from pathlib import Path

import numpy as np
import torch

from ..augmentor import augmentor_utils
from ..augmentor.database_sampler import DataBaseSampler
from ..mixup_dataset import draw_mixup_indices, encode_frame, finish_half
from ..processor.intra_domain_point_mixup import intra_domain_point_mixup_cd
from ..synthetic import SyntheticPairDataset
from .nuscenes_dataset import EGO_RADIUS, NuScenesDataset

MIXUP_TYPES = ("only_gt", "ps_gt", "gt_gt+ps", "gt+ps_gt+ps", "no_mixup")
ADV_MODIFY, ADV_ADD, ADV_REMOVE = 0, 1, 2             # op codes of ops.adv_edit; 3: nothing


def fmix32(h):
    """murmur3's 32-bit finaliser on uint32 arrays (wrapping arithmetic)."""
    h = np.atleast_1d(np.asarray(h, np.uint32)).copy()
    h ^= h >> np.uint32(16)
    h *= np.uint32(0x85EBCA6B)
    h ^= h >> np.uint32(13)
    h *= np.uint32(0xC2B2AE35)
    h ^= h >> np.uint32(16)
    return h


def subset_keys(seed, rows):
    """key(i) = fmix32(seed ^ uint32(i * 0x9E3779B9)) for the row indices `rows`: pairwise different for rows below 2^32."""
    return fmix32(np.uint32(seed) ^ (np.atleast_1d(rows).astype(np.uint32) * np.uint32(0x9E3779B9)))


def _boxes7(boxes):
    """[k, 7] fp32 copy of an info's boxes (an empty list of boxes has no second axis to keep)."""
    boxes = np.asarray(boxes, np.float32)
    return (boxes if boxes.ndim == 2 else boxes.reshape(-1, 7))[:, :7].copy()


def subset_size(frac, c):
    """c - k with k = min(floor(frac * c), c - 1), the product in float64."""
    return c - min(int(np.floor(float(frac) * c)), c - 1)


class NuScenesMixUpAdvDataset(NuScenesDataset):
    is_pair_dataset = True

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
        self.repeat = int(dataset_cfg.get("REPEAT", 0) or 0)
        self.mixup_prob = float(dataset_cfg.get("MIXUP_PROB", 0.6))
        self.mixup_type = dataset_cfg.get("MIXUP_TYPE", "gt+ps_gt+ps")
        if self.mixup_type not in MIXUP_TYPES:
            raise NotImplementedError(f"MIXUP_TYPE '{self.mixup_type}': known are {', '.join(MIXUP_TYPES)}")
        self.gt_prob = float(dataset_cfg.get("GT_PROB", 0.3))
        self.alpha = float(dataset_cfg.get("ALPHA", 2))
        self.pseudo_thresh = float(dataset_cfg.get("PSEUDO_THRESH", 0.3))
        self.adv_eps = float(dataset_cfg.get("ADV_EPS", 1e-3))
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

    def __len__(self):
        if self._merge_all_iters_to_one_epoch:
            return len(self.infos) * self.total_epochs
        if self.repeat:
            return len(self.gt_infos) * self.repeat
        return len(self.infos)

    def is_gt(self, k):
        return k < len(self.gt_infos)

    def pseudo_frame(self, info, thres=None):
        """Drops the pseudo boxes with p_score < thres (reference :30-45); a labelled info passes."""
        if "p_score" in info:
            keep = ~(np.asarray(info["p_score"]) < (self.pseudo_thresh if thres is None else thres))
            info["gt_boxes"], info["gt_names"], info["p_score"] = info["gt_boxes"][keep], info["gt_names"][keep], info["p_score"][keep]
        return info

    def frame_points(self, info):
        """[n, 5] CUDA tensor of one info: key frame and MAX_SWEEPS - 1 sweeps merged, SHIFT_COOR added."""
        from .... import ops
        paths, matrices, lags, drop_ego = self._sweep_table(info, self.max_sweeps)
        rows, offsets = self.read_rows(paths)
        shift = np.array(self.shift_coor, dtype=np.float32) if self.shift_coor else None
        out, flags = ops.sweeps_merge(torch.from_numpy(rows).cuda(), offsets, matrices, lags, drop_ego, radius=EGO_RADIUS, shift=shift)
        return ops.RowBuffer(out.shape[0], 5, out.device).append(out, flags, 1).finish()

    # ---- the adversarial edit
    @staticmethod
    def draw_edits(k):
        """The host's draws for k pseudo boxes, per box and in box order: op, frac, seed."""
        op, frac, seed = np.zeros(k, np.int64), np.zeros(k, np.float64), np.zeros(k, np.uint32)
        for j in range(k):
            op[j] = np.random.randint(3)
            frac[j] = np.random.random()
            seed[j] = np.random.randint(0, 2 ** 32, dtype=np.uint32)
        return {"op": op, "frac": frac, "seed": seed}

    def adversarial_boxes(self, info):
        """The pseudo boxes the edit visits: p_score > PSEUDO_THRESH, fp32, SHIFT_COOR added (reference :207-214)."""
        boxes = _boxes7(info["gt_boxes"])
        boxes = boxes[np.asarray(info.get("p_score", np.ones(len(boxes)))) > self.pseudo_thresh]
        if self.shift_coor:
            boxes[:, 0:3] += np.asarray(self.shift_coor, np.float32)
        return boxes

    def voxel_table(self, info):
        """(sorted int64 keys [M], fp32 gradients [M, 3]) of a pseudo info: key = (z * gy + y) * gx + x of p_voxel_coords."""
        coords = np.asarray(info["p_voxel_coords"], np.int64).reshape(-1, 3)
        grads = np.asarray(info["p_voxel_perturb"], np.float32)
        grads = np.ascontiguousarray(grads[:, :3]) if len(coords) else np.zeros((0, 3), np.float32)
        gx, gy, _ = (int(g) for g in self.grid_size)
        keys = (coords[:, 0] * gy + coords[:, 1]) * gx + coords[:, 2]
        order = np.argsort(keys, kind="stable")
        return keys[order], grads[order]

    def adversarial_points(self, points, info, draws=None):
        """The edit of reference :191-274 on a device cloud.  `draws`: draw_edits' dict (drawn here when None)."""
        from .... import ops
        if "p_voxel_perturb" not in info or len(info["gt_boxes"]) == 0:
            return points
        boxes = self.adversarial_boxes(info)
        if len(boxes) == 0:
            return points
        draws = self.draw_edits(len(boxes)) if draws is None else draws
        keys, grads = (torch.from_numpy(t).cuda() for t in self.voxel_table(info))      # sorted and uploaded once per frame
        cfg = {"point_cloud_range": self.point_cloud_range, "voxel_size": self.voxel_size, "grid_size": self.grid_size}
        return ops.adv_edit(points, boxes, draws["op"], draws["frac"], draws["seed"], keys, grads, cfg, self.adv_eps)[0]

    def voxel_gradients_host(self, xyz, info):
        """g_i of every row: the stored gradient of its voxel, zero outside the grid or for an absent key (fp32 arithmetic)."""
        keys, grads = self.voxel_table(info)
        lo, v = np.asarray(self.point_cloud_range[:3], np.float32), np.asarray(self.voxel_size, np.float32)
        grid = np.asarray([int(g) for g in self.grid_size], np.float32)
        with np.errstate(invalid="ignore"):
            cell = np.floor((xyz.astype(np.float32) - lo) / v)
            inside = ((cell >= 0) & (cell < grid)).all(1)
        cell = np.where(inside[:, None], cell, 0).astype(np.int64)
        gx, gy = int(self.grid_size[0]), int(self.grid_size[1])
        pkeys = np.where(inside, (cell[:, 2] * gy + cell[:, 1]) * gx + cell[:, 0], -1)
        out = np.zeros((len(xyz), 3), np.float32)
        if len(keys):
            pos = np.clip(np.searchsorted(keys, pkeys), 0, len(keys) - 1)
            found = keys[pos] == pkeys
            out[found] = grads[pos[found]]
        return out

    def adversarial_points_host(self, points, info, draws):
        """adversarial_points in numpy on a host cloud [n, c] with the draws passed in; rows in the device's order: the unmarked
        rows with their final coordinates, then the added rows in (row, box) order."""
        if "p_voxel_perturb" not in info or len(info["gt_boxes"]) == 0:
            return points
        boxes = self.adversarial_boxes(info)
        if len(boxes) == 0:
            return points
        d = np.float32(self.adv_eps) * self.voxel_gradients_host(points[:, :3], info)
        cur = points[:, :3].copy()
        marked = np.zeros(len(points), bool)
        added, tags = [], []
        for j, box in enumerate(boxes):
            rows = np.nonzero(augmentor_utils.get_points_in_box(points, box)[1])[0]
            op, c = int(draws["op"][j]), len(rows)
            if not ((op in (ADV_MODIFY, ADV_ADD) and c >= 1) or (op == ADV_REMOVE and c > 5)):
                continue
            picked = np.sort(rows[np.argsort(subset_keys(draws["seed"][j], rows), kind="stable")[:subset_size(draws["frac"][j], c)]])
            if op == ADV_MODIFY:
                cur[picked] = cur[picked] - d[picked]
            elif op == ADV_ADD:
                extra = points[picked].copy()
                extra[:, :3] = cur[picked] - d[picked]
                added.append(extra)
                tags.append(np.stack([picked, np.full(len(picked), j)], 1))
            else:
                marked[picked] = True
        out = points.copy()
        out[:, :3] = cur
        out = out[~marked]
        if added:
            tags = np.concatenate(tags, 0)
            out = np.concatenate([out, np.concatenate(added, 0)[np.lexsort((tags[:, 1], tags[:, 0]))]], 0)
        return out

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

    def draw_item(self, index):
        """The sampling policy: ("same", k) or ("mixup", k1, k2), indices into infos."""
        n_gt, n_ps = len(self.gt_infos), len(self.ps_infos)
        assert n_gt != 0 and n_ps != 0
        prob = np.random.random(1)
        if self.mixup_type == "no_mixup":
            return ("same", index % n_gt)
        if prob > self.mixup_prob:
            if np.random.random(1) < self.gt_prob:
                return ("same", index % n_gt)
            return ("same", n_gt + index % n_ps)
        return ("mixup",) + tuple(int(i) for i in draw_mixup_indices(self.mixup_type, n_gt + n_ps, n_gt))

    def raw_pair(self, item):
        """draw_item's choice as the (adv, org) frames, class filter, class-id column and feature encoding applied, mixed."""
        if item[0] == "same":
            return encode_frame(self, self.frame(item[1], True)), encode_frame(self, self.frame(item[1], False))
        _, k1, k2 = item
        adv = intra_domain_point_mixup_cd(encode_frame(self, self.frame(k1, True)), encode_frame(self, self.frame(k2, True)), alpha=self.alpha)
        org = intra_domain_point_mixup_cd(encode_frame(self, self.frame(k1, False)), encode_frame(self, self.frame(k2, False)), alpha=self.alpha)
        return adv, org

    def __getitem__(self, index):
        if self._merge_all_iters_to_one_epoch:
            index = index % len(self.infos)
        adv, org = self.raw_pair(self.draw_item(index))
        adv, org = finish_half(self, adv), finish_half(self, org)
        if self.dataset_cfg.get("SET_NAN_VELOCITY_TO_ZEROS", False):
            for half in (adv, org):
                half["gt_boxes"][np.isnan(half["gt_boxes"])] = 0
        if self.training and (len(adv["gt_boxes"]) == 0 or len(org["gt_boxes"]) == 0):
            return self[np.random.randint(len(self))]
        return adv, org

    collate_batch = staticmethod(SyntheticPairDataset.collate_batch)
