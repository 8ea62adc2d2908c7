"""Stage-2 dataset of TODA: (adversarial, original) pairs of target-domain frames with intra-domain MixUp
(reference pcdet/datasets/nuscenes/nuscenes_mixup_adv_dataset.py:191-274 adversarial frame, :286-588 sampling policy,
:700-760 prepare_data through intra_domain_point_mixup_cd).

Frames [0, NUM_GT) play the labelled subset (`gt_infos`), the rest the pseudo-labelled subset (`ps_infos`, labels from
PSEUDO_INFO_PATH as written by tools/generate_pseudo_labels[_perturb].py).  Per item:
  with probability 1 - MIXUP_PROB   the same frame twice: a labelled frame (probability GT_PROB) or a pseudo-labelled
                                    frame whose `adv` copy carries the adversarial point edits;
  otherwise                         a MixUp (with collision removal, on the MI355X) of two frames drawn per MIXUP_TYPE
                                    (only_gt | ps_gt | gt_gt+ps | gt+ps_gt+ps), built once for `adv` and once for `org`.
Both halves then pass the DataAugmentor independently (their flips / rotation / scaling are recorded and undone on the
predictions by the consistency loss) and the data processor.

The adversarial edit follows the reference's scheme - for every pseudo box above PSEUDO_THRESH one of modify / add /
remove (np.random.randint(3)) on a random subset of the box's points, with x' = x - eps * g, eps = 1e-3 - where g is the
stored gradient of the detection loss at the point's voxel (`p_voxel_perturb` / `p_voxel_coords` of the infos file).
The reference's lookup helpers live in a module that is not part of the repository (pcdet/utils/perturb_utils.py), so the
voxel lookup here is this build's own: key = linearised (z, y, x) voxel of the point, binary search in the stored keys."""
import numpy as np
import torch

from ..config import AttrDict
from .augmentor import augmentor_utils
from .processor.intra_domain_point_mixup import intra_domain_point_mixup_cd
from .synthetic import SyntheticPairDataset


def draw_mixup_indices(mixup_type, n, n_gt):
    """The two frames of a MixUp item out of n frames, the first n_gt of them labelled: two np.random.randint calls."""
    if mixup_type == "only_gt":
        return np.random.randint(n_gt), np.random.randint(n_gt)
    if mixup_type == "ps_gt":
        return n_gt + np.random.randint(n - n_gt), np.random.randint(n_gt)
    if mixup_type == "gt_gt+ps":
        return np.random.randint(n_gt), np.random.randint(n)
    if mixup_type == "gt+ps_gt+ps":
        return np.random.randint(n), np.random.randint(n)
    raise NotImplementedError(mixup_type)


def encode_frame(dataset, data):
    """Class filter + class-id column + feature encoding - what prepare_data does before the mix.  gt_names leave: from here on
    the class of a box is column 7 of gt_boxes; every other key of `data` passes."""
    names = data["gt_names"]
    keep = np.array([n in dataset.class_names for n in names], dtype=bool)
    ids = np.array([dataset.class_names.index(n) + 1 for n in names[keep]], dtype=np.float32).reshape(-1, 1)
    out = {k: v for k, v in data.items() if k != "gt_names"}
    out["gt_boxes"] = np.concatenate([data["gt_boxes"][keep], ids], axis=1).astype(np.float32)
    return dataset.point_feature_encoder.forward(out)


def finish_half(dataset, data):
    """One half of a pair after the mix: DataAugmentor (records its transforms), then the processor queue.  The augmentor sees
    boxes [n, 7] with their names and an all-true gt_boxes_mask, as prepare_data hands them over, so gt_sampling can paste; the
    class-id column is rebuilt from the names that come back, which gives the pasted boxes theirs."""
    if dataset.training and dataset.data_augmentor is not None:
        names = np.array(dataset.class_names)[data["gt_boxes"][:, 7].astype(np.int64) - 1]
        aug = dataset.data_augmentor.forward({"points": data["points"], "gt_boxes": data["gt_boxes"][:, :7].copy(), "gt_names": names,
                                              "gt_boxes_mask": np.ones(len(names), dtype=bool)})
        ids = np.array([dataset.class_names.index(n) + 1 for n in aug["gt_names"]], dtype=np.float32).reshape(-1, 1)
        data.update(points=aug["points"], gt_boxes=np.concatenate([aug["gt_boxes"], ids], 1).astype(np.float32),
                    augmentation_list=aug.get("augmentation_list", []), augmentation_params=aug.get("augmentation_params", {}))
    else:
        data.setdefault("augmentation_list", [])
        data.setdefault("augmentation_params", {})
    return dataset.data_processor.forward(data)


class SyntheticMixupPairDataset(SyntheticPairDataset):
    def __init__(self, dataset_cfg, class_names, training=True, root_path=None, logger=None):
        super().__init__(dataset_cfg=dataset_cfg, class_names=class_names, training=training, root_path=root_path, logger=logger)
        self.num_gt = int(dataset_cfg.get("SYNTHETIC", AttrDict()).get("NUM_GT", self.num_samples // 2))
        self.mixup_prob = float(dataset_cfg.get("MIXUP_PROB", 0.6))
        self.mixup_type = dataset_cfg.get("MIXUP_TYPE", "gt+ps_gt+ps")
        self.gt_prob = float(dataset_cfg.get("GT_PROB", 0.5))
        self.alpha = float(dataset_cfg.get("ALPHA", 2))
        self.pseudo_thresh = float(dataset_cfg.get("PSEUDO_THRESH", 0.3))
        self.adv_eps = float(dataset_cfg.get("ADV_EPS", 1e-3))
        self.on_device = bool(dataset_cfg.get("MIX_ON_DEVICE", True))

    # ---- frames ---------------------------------------------------------------------------
    def is_gt(self, index):
        return index < self.num_gt

    def frame(self, index, adversarial):
        points, boxes, names = self.raw_sample(index, use_pseudo=not self.is_gt(index))
        points = points.copy()
        if adversarial and not self.is_gt(index) and self.pseudo_infos is not None:
            points = self.adversarial_points(points, self.pseudo_infos[self.frame_id(index)])
        return {"points": points, "gt_boxes": boxes.copy(), "gt_names": names.copy(), "frame_id": self.frame_id(index)}

    def voxel_keys(self, xyz):
        r, v = self.point_cloud_range, np.asarray(self.voxel_size, np.float32)
        cell = np.floor((xyz - r[0:3]) / v).astype(np.int64)                       # (x, y, z) cell
        gx, gy, gz = (int(g) for g in self.grid_size)
        inside = ((cell >= 0) & (cell < np.array([gx, gy, gz]))).all(1)
        return np.where(inside, (cell[:, 2] * gy + cell[:, 1]) * gx + cell[:, 0], -1)

    def adversarial_points(self, points, info):
        """Reference get_ps_adv_lidar_with_sweeps (:191-274) on one cloud."""
        if "p_voxel_perturb" not in info or len(info["gt_boxes"]) == 0:
            return points
        coords = np.asarray(info["p_voxel_coords"], np.int64)                      # [M, 3] (z, y, x)
        grads = np.asarray(info["p_voxel_perturb"], np.float32)[:, :3]
        gx, gy, _ = (int(g) for g in self.grid_size)
        keys = (coords[:, 0] * gy + coords[:, 1]) * gx + coords[:, 2]
        order = np.argsort(keys)
        keys, grads = keys[order], grads[order]
        pkeys = self.voxel_keys(points[:, :3])
        pos = np.clip(np.searchsorted(keys, pkeys), 0, max(len(keys) - 1, 0))
        found = (len(keys) > 0) & (keys[pos] == pkeys) if len(keys) else np.zeros(len(points), bool)
        perturb = np.where(found[:, None], grads[pos], 0.0).astype(np.float32)
        scores = np.asarray(info.get("p_score", np.ones(len(info["gt_boxes"]))))
        removed = []
        for box in np.asarray(info["gt_boxes"], np.float32)[scores > self.pseudo_thresh]:
            p_idx = np.nonzero(augmentor_utils.get_points_in_box(points, box)[1])[0]
            kind = np.random.randint(3)
            if kind in (0, 1) and len(p_idx) > 0:
                moved = points[p_idx, :3] - self.adv_eps * perturb[p_idx]
                k = np.random.randint(len(p_idx))
                pick = np.arange(len(p_idx))
                np.random.shuffle(pick)
                pick = pick[k:]
                if kind == 0:                                                       # modify
                    points[p_idx[pick], :3] = moved[pick]
                else:                                                               # add displaced copies
                    extra = points[p_idx[pick]].copy()
                    extra[:, :3] = moved[pick]
                    points = np.concatenate([points, extra], 0)
                    perturb = np.concatenate([perturb, np.zeros((len(extra), 3), np.float32)], 0)
            elif kind == 2 and len(p_idx) > 5:                                      # remove
                k = np.random.randint(len(p_idx))
                pick = np.arange(len(p_idx))
                np.random.shuffle(pick)
                removed.append(p_idx[pick[k:]])
        if removed:
            points = np.delete(points, np.concatenate(removed), axis=0)
        return points

    # ---- sampling policy --------------------------------------------------------------------
    def draw_mixup_indices(self):
        return draw_mixup_indices(self.mixup_type, self.num_samples, self.num_gt)

    def _encode(self, data):
        """encode_frame after the upload."""
        return encode_frame(self, {**data, "points": torch.from_numpy(data["points"]).cuda() if self.on_device else data["points"]})

    def _finish(self, data):
        return finish_half(self, data)

    def __getitem__(self, index):
        index = index % self.num_samples
        if np.random.random(1) > self.mixup_prob or self.mixup_type == "no_mixup":
            if self.mixup_type == "no_mixup" or np.random.random(1) < self.gt_prob:
                src = index % max(self.num_gt, 1)
            else:
                src = self.num_gt + index % max(self.num_samples - self.num_gt, 1)
            adv, org = self._encode(self.frame(src, True)), self._encode(self.frame(src, False))
        else:
            i1, i2 = self.draw_mixup_indices()
            adv = intra_domain_point_mixup_cd(self._encode(self.frame(i1, True)), self._encode(self.frame(i2, True)), alpha=self.alpha)
            org = intra_domain_point_mixup_cd(self._encode(self.frame(i1, False)), self._encode(self.frame(i2, False)), alpha=self.alpha)
        adv, org = self._finish(adv), self._finish(org)
        if self.training and (len(adv["gt_boxes"]) == 0 or len(org["gt_boxes"]) == 0):
            return self[np.random.randint(len(self))]
        return adv, org


# --------------------------------------------------------------------------------------------------------------------------
# The stage-2 pair policy and the adversarial edit of the datasets that read real frames (NuScenesMixUpAdvDataset,
# KittiMixUpAdvDataset).  Neither depends on the dataset: the class below is mixed into both in front of their dataset class,
# which supplies infos = gt_infos + ps_infos, is_gt(k), frame(k, adversarial, draws), shift_coor, point_cloud_range, voxel_size
# and grid_size.
# --------------------------------------------------------------------------------------------------------------------------
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


class MixUpAdvPairPolicy:
    is_pair_dataset = True

    def init_pair_policy(self, dataset_cfg, pseudo_thresh=0.3):
        """The mixup keys of the dataset config; `pseudo_thresh`: the class's default for PSEUDO_THRESH."""
        self.repeat = int(dataset_cfg.get("REPEAT", 0) or 0)
        self.mixup_prob = float(dataset_cfg.get("MIXUP_PROB", 0.6))
        self.mixup_type = dataset_cfg.get("MIXUP_TYPE", "gt+ps_gt+ps")
        if self.mixup_type not in MIXUP_TYPES:
            raise NotImplementedError(f"MIXUP_TYPE '{self.mixup_type}': known are {', '.join(MIXUP_TYPES)}")
        self.gt_prob = float(dataset_cfg.get("GT_PROB", 0.3))
        self.alpha = float(dataset_cfg.get("ALPHA", 2))
        self.pseudo_thresh = float(dataset_cfg.get("PSEUDO_THRESH", pseudo_thresh))
        self.adv_eps = float(dataset_cfg.get("ADV_EPS", 1e-3))

    def __len__(self):
        if self._merge_all_iters_to_one_epoch:
            return len(self.infos) * self.total_epochs
        if self.repeat:
            return len(self.gt_infos) * self.repeat
        return len(self.infos)

    def is_gt(self, k):
        return k < len(self.gt_infos)

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
        from ... import ops
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

    # ---- items
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
