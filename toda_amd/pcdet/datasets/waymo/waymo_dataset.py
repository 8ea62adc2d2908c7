"""WaymoDataset (behaviour of reference pcdet/datasets/waymo/waymo_dataset.py): the processed Waymo Open Dataset frames on disk
and the per-sequence info pickles of a stock OpenPCDet preparation (v0.5.0) -> training / evaluation samples, the GT-sampling
database, prediction dicts, the KITTI-style AP and the Waymo LEVEL_1 / LEVEL_2 AP / APH (eval_metric 'aph', waymo_eval.py).

    <DATA_PATH>/ImageSets/{train,val}.txt                                   one sequence per line (segment-..._with_camera_labels.tfrecord)
    <DATA_PATH>/<PROCESSED_DATA_TAG>/<sequence>/<sequence>.pkl              list of {point_cloud {lidar_sequence, sample_idx}, frame_id,
                                                                            annos {name, difficulty, gt_boxes_lidar, num_points_in_gt}, ...}
    <DATA_PATH>/<PROCESSED_DATA_TAG>/<sequence>/%04d.npy                    [n, 6] fp32: x, y, z, intensity, elongation, NLZ flag
    <DATA_PATH>/<OTHER_CHANNEL>/<sequence>/%04d.npy                         the frames, when OTHER_CHANNEL is set (e.g. modes/16^)

MI355X layout: a frame goes to the device in one H2D copy, one kernel pass (ops.waymo_frame, csrc/waymo_frame.hip) writes
x, y, z, tanh(intensity), elongation and flags the rows outside the no-label zones (NLZ flag == -1); the stable compaction
(ops.RowBuffer) drops the others - skipped with DISABLE_NLZ_FLAG_ON_POINTS - and the range mask, the shuffle and the voxeliser
of the data processor follow on the device.  The reference does this in numpy inside DataLoader workers.  Samples are CUDA
tensors (`on_device`): build_dataloader runs the dataset in the training process, no worker process opens the GPU.
get_lidar_host is the same work in the reference's numpy statements: the test oracle and the bench baseline.  The kernel's
intensity is (float)tanh((double)i), the correctly rounded value; numpy's fp32 tanh lies within an ulp of it.

Not built: the info builder from TFRecords (create_waymo_infos; it needs TensorFlow and the waymo_open_dataset package), the
estimator route of the Waymo L1 / L2 metric (eval_metric 'waymo' raises ImportError naming those packages; eval_metric 'aph' is
the same metric on the project's own kernels, eval_metric 'kitti' the KITTI table), and the shared-memory frame cache: USE_SHARED_MEMORY of the dataset is accepted and ignored, frames already live in HBM.

    python -m toda_amd.pcdet.datasets.waymo.waymo_dataset create_waymo_gt_database <dataset yaml> [--data_path DIR] [--processed_data_tag TAG]
"""
import copy
import os
import pickle
from pathlib import Path

import numpy as np
import torch

from ...utils import box_utils, common_utils
from ..dataset import DatasetTemplate, lidar_kitti_eval, lidar_prediction_dicts

MAP_NAME_TO_KITTI = {"Vehicle": "Car", "Pedestrian": "Pedestrian", "Cyclist": "Cyclist", "Sign": "Sign", "Car": "Car"}
FRAME_COLS_MIN = 6               # x, y, z, intensity, elongation, NLZ flag


class WaymoDataset(DatasetTemplate):
    on_device = True             # samples leave __getitem__ as CUDA tensors: build_dataloader keeps the dataset in the training process

    def __init__(self, dataset_cfg, class_names, training=True, root_path=None, logger=None):
        super().__init__(dataset_cfg=dataset_cfg, class_names=class_names, training=training, root_path=root_path, logger=logger)
        self.root_path = Path(self.root_path)
        self.data_path = self.root_path / dataset_cfg.PROCESSED_DATA_TAG
        other = dataset_cfg.get("OTHER_CHANNEL", None)
        self.frame_path = self.root_path / other if other else self.data_path
        self.use_nlz = not dataset_cfg.get("DISABLE_NLZ_FLAG_ON_POINTS", False)
        self.set_split(dataset_cfg.DATA_SPLIT[self.mode])

    # ---- reading
    def set_split(self, split):
        self.split = split
        with open(self.root_path / "ImageSets" / (split + ".txt")) as f:
            self.sample_sequence_list = [line.strip() for line in f.readlines()]
        self.infos = []
        self.include_waymo_data(self.mode)

    @staticmethod
    def check_sequence_name_with_all_version(sequence_file):
        """The file as the list names it or, when that does not exist, under the names other releases of the dataset use:
        `segment` with a training_ / validation_ / testing_ prefix, else without `_with_camera_labels`.  A miss returns the
        argument."""
        if sequence_file.exists():
            return sequence_file
        found = sequence_file
        for prefix in ("training", "validation", "testing"):
            candidate = Path(str(sequence_file).replace("segment", prefix + "_segment"))
            if candidate.exists():
                found = candidate
                break
        if not found.exists():
            found = Path(str(sequence_file).replace("_with_camera_labels", ""))
        return found if found.exists() else sequence_file

    def include_waymo_data(self, mode):
        self._log("Loading Waymo dataset")
        infos, self.num_skipped_infos = [], 0
        for line in self.sample_sequence_list:
            name = os.path.splitext(line)[0]
            path = self.check_sequence_name_with_all_version(self.data_path / name / f"{name}.pkl")
            if not path.exists():
                self.num_skipped_infos += 1
                continue
            with open(path, "rb") as f:
                infos.extend(pickle.load(f))
        self._log("Total skipped info %s" % self.num_skipped_infos)
        self._log("Total samples for Waymo dataset: %d" % len(infos))
        interval = int(self.dataset_cfg.SAMPLED_INTERVAL[mode])
        if interval > 1:
            infos = infos[::interval]
            self._log("Total sampled samples for Waymo dataset: %d" % len(infos))
        self.infos.extend(infos)

    def read_frame(self, sequence_name, sample_idx):
        """[n, c >= 6] fp32 rows of a frame file, as they are on disk."""
        path = self.frame_path / sequence_name / ("%04d.npy" % sample_idx)
        rows = np.load(path)
        if rows.ndim != 2 or rows.dtype != np.float32 or rows.shape[1] < FRAME_COLS_MIN:
            raise ValueError(f"{path}: {rows.dtype} array of shape {rows.shape}, a processed frame is [n, {FRAME_COLS_MIN} or more] float32 "
                             "(x, y, z, intensity, elongation, NLZ flag)")
        return rows

    def get_lidar(self, sequence_name, sample_idx):
        """[n', 5] CUDA tensor (x, y, z, tanh(intensity), elongation): the rows with NLZ flag == -1 in file order, or every row
        with DISABLE_NLZ_FLAG_ON_POINTS.  One upload, one kernel pass, one compaction."""
        from .... import ops
        rows = np.ascontiguousarray(self.read_frame(sequence_name, sample_idx))
        out, flags = ops.waymo_frame(torch.from_numpy(rows).cuda(), use_nlz=self.use_nlz)
        if not self.use_nlz:
            return out
        return ops.RowBuffer(out.shape[0], 5, out.device).append(out, flags, 1).finish()

    def get_lidar_host(self, sequence_name, sample_idx):
        """get_lidar in numpy, the reference's statements: [n', 5] fp32."""
        point_features = self.read_frame(sequence_name, sample_idx)
        points_all, nlz_flag = point_features[:, 0:5], point_features[:, 5]
        if self.use_nlz:
            points_all = points_all[nlz_flag == -1]
        points_all[:, 3] = np.tanh(points_all[:, 3])
        return points_all

    # ---- samples
    def raw_frame(self, index, host=False):
        """Frame `index` before prepare_data: {points, frame_id, metadata} and, with annotations, gt_names / gt_boxes /
        num_points_in_gt without the `unknown` objects (and, in training with FILTER_EMPTY_BOXES_FOR_TRAIN, without the empty
        boxes).  host: the points through get_lidar_host."""
        info = copy.deepcopy(self.infos[index])
        pc_info = info["point_cloud"]
        read = self.get_lidar_host if host else self.get_lidar
        data = {"points": read(pc_info["lidar_sequence"], pc_info["sample_idx"]), "frame_id": info["frame_id"],
                "metadata": info.get("metadata", info["frame_id"])}
        if "annos" in info:
            annos = common_utils.drop_info_with_name(info["annos"], name="unknown")
            boxes = annos["gt_boxes_lidar"]
            if self.dataset_cfg.get("INFO_WITH_FAKELIDAR", False):
                boxes = box_utils.boxes3d_kitti_fakelidar_to_lidar(boxes)
            if self.training and self.dataset_cfg.get("FILTER_EMPTY_BOXES_FOR_TRAIN", False):
                mask = annos["num_points_in_gt"] > 0
                annos["name"], boxes, annos["num_points_in_gt"] = annos["name"][mask], boxes[mask], annos["num_points_in_gt"][mask]
            data.update(gt_names=annos["name"], gt_boxes=boxes, num_points_in_gt=annos.get("num_points_in_gt", None))
        return data

    def __getitem__(self, index):
        if self._merge_all_iters_to_one_epoch:
            index = index % len(self.infos)
        data = self.raw_frame(index)
        metadata = data.pop("metadata")
        data = self.prepare_data(data)
        data["metadata"] = metadata
        data.pop("num_points_in_gt", None)
        if self.training and "gt_boxes" in data and len(data["gt_boxes"]) == 0:        # reference dataset.py:152-154
            return self[np.random.randint(len(self))]
        return data

    # ---- predictions
    @staticmethod
    def generate_prediction_dicts(batch_dict, pred_dicts, class_names, output_path=None):
        """Per frame {name, score, boxes_lidar, frame_id, metadata}; a frame without detections keeps the zero-length float
        fields of the reference's template."""
        return lidar_prediction_dicts(batch_dict, pred_dicts, class_names, with_labels=False)

    def evaluation(self, det_annos, class_names, **kwargs):
        if not self.infos or "annos" not in self.infos[0]:
            return "No ground-truth boxes for evaluation", {}
        metric = kwargs.get("eval_metric", None)
        if metric == "kitti":
            gt_annos = [common_utils.drop_info_with_name(copy.deepcopy(info["annos"]), name="unknown") for info in self.infos]
            return self.kitti_eval(copy.deepcopy(det_annos), gt_annos, class_names)
        if metric == "aph":
            return self.aph_eval(det_annos, class_names, route=kwargs.get("eval_route", "device"))
        if metric == "waymo":
            return self.waymo_eval(det_annos, class_names, **kwargs)
        raise NotImplementedError(f"eval_metric '{metric}': WaymoDataset scores with 'kitti', 'aph' (or 'waymo' through the Waymo Open Dataset estimator)")

    def kitti_eval(self, eval_det_annos, eval_gt_annos, class_names):
        """The KITTI AP table in the LiDAR frame: detections and infos pair up by position, Vehicle scores as Car, every object
        gets the placeholder image box (so all are Easy); INFO_WITH_FAKELIDAR applies to the ground truth only.  `unknown`
        objects, which have no KITTI name, are left out of the ground truth (a stock preparation stores none)."""
        return lidar_kitti_eval(eval_det_annos, eval_gt_annos, MAP_NAME_TO_KITTI, [MAP_NAME_TO_KITTI[c] for c in class_names],
                                info_with_fakelidar=self.dataset_cfg.get("INFO_WITH_FAKELIDAR", False))

    def aph_eval(self, det_annos, class_names, route="device"):
        """LEVEL_1 / LEVEL_2 AP and APH per object type (waymo_eval.py): detections and infos pair up by position;
        neither is changed.  route 'host' is the numpy / scipy statement of the same metric."""
        from . import waymo_eval
        return waymo_eval.evaluate(det_annos, [info["annos"] for info in self.infos], class_names,
                                   info_with_fakelidar=self.dataset_cfg.get("INFO_WITH_FAKELIDAR", False), route=route)

    def waymo_eval(self, det_annos, class_names, **kwargs):
        try:
            import tensorflow  # noqa: F401
            import waymo_open_dataset  # noqa: F401
        except ImportError as e:
            raise ImportError("eval_metric 'waymo' (L1 / L2 AP and APH) runs the detection metrics estimator of the Waymo Open Dataset "
                              "(packages tensorflow and waymo-open-dataset, modules `tensorflow` and `waymo_open_dataset`), which are "
                              "not installed; score with eval_metric 'aph' (the same metric on this project's kernels) or 'kitti' instead") from e
        raise NotImplementedError("the Waymo Open Dataset estimator is not wired up: score with eval_metric 'aph' or 'kitti'")

    # ---- GT database: the frames of an infos pickle through augmentor/database_sampler.create_groundtruth_database
    def create_groundtruth_database(self, info_path, save_path, used_classes=None, split="train", sampled_interval=10,
                                    processed_data_tag=None):
        """<tag>_gt_database_<split>_sampled_<k>/<sequence>_%04d_<class>_<i>.bin for the objects of a used class,
        <tag>_waymo_dbinfos_<split>_sampled_<k>.pkl and <tag>_gt_database_<split>_sampled_<k>_global.npy under save_path, from every
        sampled_interval-th frame of the infos pickle.  Vehicle boxes are taken from every 4th frame of the pickle only and
        Pedestrian boxes from every 2nd, as in the reference."""
        from ..augmentor.database_sampler import create_groundtruth_database
        with open(info_path, "rb") as f:
            infos = pickle.load(f)
        frames = _InfoFrames(self, infos, sampled_interval)
        stem = "%s_gt_database_%s_sampled_%d" % (processed_data_tag, split, sampled_interval)
        return create_groundtruth_database(frames, Path(save_path), used_classes=used_classes, packed=True, db_name=stem,
                                           info_name="%s_waymo_dbinfos_%s_sampled_%d.pkl" % (processed_data_tag, split, sampled_interval),
                                           frame_id=frames.frame_id, extra_info=frames.extra_info, files_for_used_only=True)


class _InfoFrames:
    """Every `interval`-th frame of an infos list as database_sampler.create_groundtruth_database reads a dataset: len(),
    raw_sample(j) -> (points [n, 5] numpy, gt_boxes, gt_names) after the reference's thinning by the frame's position k in the
    list (Vehicle only where k % 4 == 0, Pedestrian only where k % 2 == 0), frame_id(j) and extra_info(j, i)."""

    def __init__(self, dataset, infos, interval):
        self.dataset, self.infos, self.picks = dataset, infos, list(range(0, len(infos), interval))

    def __len__(self):
        return len(self.picks)

    def thinned(self, j):
        k = self.picks[j]
        annos = self.infos[k]["annos"]
        keep = np.ones(len(annos["name"]), bool)
        if k % 4 != 0:
            keep &= annos["name"] != "Vehicle"
        if k % 2 != 0:
            keep &= annos["name"] != "Pedestrian"
        return annos["name"][keep], annos["difficulty"][keep], annos["gt_boxes_lidar"][keep]

    def raw_sample(self, j):
        pc_info = self.infos[self.picks[j]]["point_cloud"]
        names, _, boxes = self.thinned(j)
        return self.dataset.get_lidar(pc_info["lidar_sequence"], pc_info["sample_idx"]).cpu().numpy(), boxes, names

    def frame_id(self, j):
        pc_info = self.infos[self.picks[j]]["point_cloud"]
        return "%s_%04d" % (pc_info["lidar_sequence"], pc_info["sample_idx"])

    def extra_info(self, j, i):
        pc_info = self.infos[self.picks[j]]["point_cloud"]
        return {"sequence_name": pc_info["lidar_sequence"], "sample_idx": pc_info["sample_idx"], "difficulty": self.thinned(j)[1][i]}


def main(argv=None):
    import argparse

    from ...config import AttrDict, cfg_from_yaml_file
    ap = argparse.ArgumentParser()
    ap.add_argument("command", choices=["create_waymo_gt_database", "create_waymo_infos"])
    ap.add_argument("cfg_file", help="dataset yaml, e.g. toda_amd/tools/cfgs/dataset_configs/waymo_dataset.yaml")
    ap.add_argument("--data_path", default=None, help="Waymo root (the directory that holds ImageSets and the processed data); default: DATA_PATH of the yaml")
    ap.add_argument("--processed_data_tag", default=None, help="default: PROCESSED_DATA_TAG of the yaml")
    args = ap.parse_args(argv)
    if args.command == "create_waymo_infos":
        raise SystemExit("create_waymo_infos is out of scope: the info builder reads the TFRecords of the Waymo Open Dataset (TensorFlow, "
                         "waymo_open_dataset).  Prepare <PROCESSED_DATA_TAG>/<sequence>/{<sequence>.pkl, %04d.npy} with a stock OpenPCDet "
                         "installation; they are read as they are, and create_waymo_gt_database builds the GT-sampling database from them.")
    dataset_cfg = cfg_from_yaml_file(args.cfg_file, AttrDict())
    if args.processed_data_tag:
        dataset_cfg.PROCESSED_DATA_TAG = args.processed_data_tag
    dataset_cfg.pop("DATA_AUGMENTOR", None)          # the sampler would look for the database that is being built
    dataset_cfg.SAMPLED_INTERVAL = AttrDict({"train": 1, "test": 1})
    tag, root = dataset_cfg.PROCESSED_DATA_TAG, Path(args.data_path or dataset_cfg.DATA_PATH)
    dataset = WaymoDataset(dataset_cfg, class_names=["Vehicle", "Pedestrian", "Cyclist"], root_path=root, training=True)
    info_path = root / ("%s_infos_%s.pkl" % (tag, dataset.split))
    if not info_path.exists():                       # the list create_waymo_infos leaves: every frame of the split's sequences
        with open(info_path, "wb") as f:
            pickle.dump(dataset.infos, f)
    db = dataset.create_groundtruth_database(info_path, root, used_classes=["Vehicle", "Pedestrian", "Cyclist"], split=dataset.split,
                                             sampled_interval=1, processed_data_tag=tag)
    for name, entries in db.items():
        print("Database %s: %d" % (name, len(entries)))


if __name__ == "__main__":
    main()
