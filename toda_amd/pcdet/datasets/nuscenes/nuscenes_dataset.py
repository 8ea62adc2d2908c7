"""NuScenesDataset (behaviour of reference pcdet/datasets/nuscenes/nuscenes_dataset.py): the nuScenes LiDAR sweeps on disk and
the info pickles of a stock OpenPCDet preparation -> training / evaluation samples, the GT-sampling database, prediction dicts
and the KITTI-style AP.

    <DATA_PATH>/<VERSION>/{samples,sweeps}/LIDAR_TOP/*.pcd.bin          [-1, 5] fp32: x, y, z, intensity, ring
    <DATA_PATH>/<VERSION>/nuscenes_infos_10sweeps_{train,val}.pkl       list of {lidar_path, token, sweeps[{lidar_path,
                                                                        transform_matrix, time_lag, ...}], gt_boxes [n, 9],
                                                                        gt_names, num_lidar_pts, ...}

MI355X layout: a sample is the key frame and MAX_SWEEPS - 1 earlier sweeps.  The files are read into one host buffer, go to
the device in one H2D copy, and one kernel pass (ops.sweeps_merge, csrc/nuscenes_frame.hip) flags the ego vehicle's points,
moves every sweep into the key frame (fp64 product, one rounding to fp32), adds SHIFT_COOR and stamps the time lag; the stable
compaction (ops.RowBuffer) drops the flagged rows, and the range mask, the shuffle and the voxeliser of the data processor
follow on the device.  The reference does this per sweep in numpy inside DataLoader workers.  With MAX_SWEEPS > 1 the samples
are CUDA tensors (`on_device`): build_dataloader then runs the dataset in the training process, no worker process opens the
GPU.  With MAX_SWEEPS == 1 there is nothing to merge: the key frame stays numpy and reaches the device with the batch.
get_lidar_with_sweeps_host is the same work in the reference's numpy arithmetic: the test oracle and the bench baseline.

Out of scope, because they walk the nuScenes devkit's tables: the info builder (create_nuscenes_infos) and the devkit's own
evaluator (eval_metric 'nuscenes' raises ImportError without the devkit).  eval_metric 'kitti' is served, and eval_metric 'nds'
is the nuScenes mAP / NDS by the project's evaluator (nuscenes_eval.py, matching on the device).

    python -m toda_amd.pcdet.datasets.nuscenes.nuscenes_dataset create_nuscenes_gt_database <dataset yaml> [--data_path DIR] [--version V]
"""
import copy
import os
import pickle
from pathlib import Path

import numpy as np
import torch

from ..dataset import DatasetTemplate

MAP_NAME_TO_KITTI = {"car": "Car", "pedestrian": "Pedestrian", "truck": "Truck"}
EGO_RADIUS = 1.0                 # half side of the square around the sensor that holds the ego vehicle's own returns
ROW_BYTES = 20                   # x, y, z, intensity, ring as fp32


class NuScenesDataset(DatasetTemplate):
    def __init__(self, dataset_cfg, class_names, training=True, root_path=None, logger=None):
        root_path = Path(root_path if root_path is not None else dataset_cfg.DATA_PATH) / dataset_cfg.VERSION
        super().__init__(dataset_cfg=dataset_cfg, class_names=class_names, training=training, root_path=root_path, logger=logger)
        self.max_sweeps = int(dataset_cfg.get("MAX_SWEEPS", 1))
        self.shift_coor = dataset_cfg.get("SHIFT_COOR", None)
        # samples leave __getitem__ as CUDA tensors: build_dataloader keeps such a dataset in the training process
        self.on_device = self.max_sweeps > 1
        self.infos = []
        self.include_nuscenes_data(self.mode)
        if self.training and dataset_cfg.get("BALANCED_RESAMPLING", False):
            self.infos = self.balanced_infos_resampling(self.infos)

    def _log(self, text):
        if self.logger is not None:
            self.logger.info(text)

    # ---- reading
    def include_nuscenes_data(self, mode):
        self._log("Loading NuScenes dataset")
        for rel in self.dataset_cfg.INFO_PATH[mode]:
            path = self.root_path / rel
            if not path.exists():
                continue
            with open(path, "rb") as f:
                self.infos.extend(pickle.load(f))
        interval = int((self.dataset_cfg.get("SAMPLED_INTERVAL", None) or {}).get(mode, 1))
        if interval > 1:
            self.infos = self.infos[::interval]
        self._log("Total samples for NuScenes dataset: %d" % len(self.infos))

    def balanced_infos_resampling(self, infos):
        """Class-balanced grouping and sampling (CBGS, arXiv 1908.09492): every class draws, with replacement, the number of
        frames that gives it 1 / len(class_names) of the class-frame pairs.  One np.random.choice per class, in class order, over
        that class's frames in info order - the reference's calls, so a seeded run picks the same frames."""
        if self.class_names is None:
            return infos
        frames_of = {name: [] for name in self.class_names}
        for info in infos:
            for name in set(info["gt_names"]):
                if name in frames_of:
                    frames_of[name].append(info)
        pairs = sum(len(v) for v in frames_of.values())
        frac = 1.0 / len(self.class_names)
        sampled = []
        for frames in frames_of.values():
            if not frames:              # a class without a frame draws nothing (the reference divides by zero here)
                continue
            ratio = frac / (len(frames) / pairs)
            sampled += np.random.choice(frames, int(len(frames) * ratio)).tolist()
        self._log("Total samples after balanced resampling: %s" % len(sampled))
        return sampled

    def _sweep_table(self, info, max_sweeps):
        """The files of a sample, key frame first, then max_sweeps - 1 of the info's sweeps in the order np.random.choice
        draws them: (paths, matrices, time lags, drop-ego flags)."""
        picks = np.random.choice(len(info["sweeps"]), max_sweeps - 1, replace=False)
        sweeps = [info["sweeps"][k] for k in picks]
        return ([self.root_path / info["lidar_path"]] + [self.root_path / s["lidar_path"] for s in sweeps],
                [None] + [s["transform_matrix"] for s in sweeps], [0.0] + [s["time_lag"] for s in sweeps], [False] + [True] * len(sweeps))

    @staticmethod
    def read_rows(paths):
        """The raw rows of the files in one host buffer: ([n, 5] fp32, row offsets per file)."""
        counts = []
        for path in paths:
            size = os.path.getsize(path)
            if size % ROW_BYTES:
                raise ValueError(f"{path}: {size} bytes is not a whole number of {ROW_BYTES}-byte rows (x, y, z, intensity, ring)")
            counts.append(size // ROW_BYTES)
        offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        rows = np.empty((int(offsets[-1]), 5), np.float32)
        for path, lo, hi in zip(paths, offsets[:-1], offsets[1:]):
            if hi > lo:
                with open(path, "rb") as f:
                    got = f.readinto(memoryview(rows[lo:hi]).cast("B"))
                if got != (hi - lo) * ROW_BYTES:
                    raise ValueError(f"{path}: short read")
        return rows, [int(o) for o in offsets]

    def get_lidar_with_sweeps(self, index, max_sweeps=1, shift=None):
        """[n, 5] CUDA tensor (x, y, z, intensity, time lag): the key frame, then the drawn sweeps without the ego vehicle's
        points, in the key frame's coordinates, `shift` (SHIFT_COOR) added.  One upload, one kernel pass, one compaction."""
        from .... import ops
        paths, matrices, lags, drop_ego = self._sweep_table(self.infos[index], max_sweeps)
        rows, offsets = self.read_rows(paths)
        dev = torch.from_numpy(rows).cuda()
        out, flags = ops.sweeps_merge(dev, offsets, matrices, lags, drop_ego, radius=EGO_RADIUS, shift=shift)
        return ops.RowBuffer(out.shape[0], 5, out.device).append(out, flags, 1).finish()

    @staticmethod
    def get_sweep_host(path, matrix, time_lag, radius=EGO_RADIUS):
        """One earlier sweep in numpy, the reference's arithmetic: ego cut on the raw coordinates, float64 product with the
        homogeneous points assigned into the fp32 cloud, a float64 time column."""
        pts = np.fromfile(str(path), dtype=np.float32).reshape(-1, 5)[:, :4]
        pts = pts[~((np.abs(pts[:, 0]) < radius) & (np.abs(pts[:, 1]) < radius))]
        if matrix is not None:
            hom = np.concatenate([pts[:, :3].T, np.ones((1, pts.shape[0]))], axis=0)
            pts[:, :3] = np.asarray(matrix).dot(hom)[:3].T
        return pts, np.full((pts.shape[0], 1), time_lag, dtype=np.float64)

    def get_lidar_with_sweeps_host(self, index, max_sweeps=1):
        """get_lidar_with_sweeps in numpy without the shift (the reference's route): [n, 5] fp32."""
        paths, matrices, lags, _ = self._sweep_table(self.infos[index], max_sweeps)
        key = np.fromfile(str(paths[0]), dtype=np.float32).reshape(-1, 5)[:, :4]
        clouds, times = [key], [np.zeros((key.shape[0], 1))]
        for path, matrix, lag in zip(paths[1:], matrices[1:], lags[1:]):
            pts, stamp = self.get_sweep_host(path, matrix, lag)
            clouds.append(pts)
            times.append(stamp)
        points = np.concatenate(clouds, axis=0)
        return np.concatenate([points, np.concatenate(times, axis=0).astype(points.dtype)], axis=1)

    # ---- samples
    def __len__(self):
        if self._merge_all_iters_to_one_epoch:
            return len(self.infos) * self.total_epochs
        return len(self.infos)

    def raw_frame(self, index):
        """Sample `index` before prepare_data: {points (SHIFT_COOR added), frame_id, metadata} and, with annotations, gt_names /
        gt_boxes [n, 9] (FILTER_MIN_POINTS_IN_GT applied, SHIFT_COOR added)."""
        info = copy.deepcopy(self.infos[index])
        shift = np.array(self.shift_coor, dtype=np.float32) if self.shift_coor else None
        if self.on_device:
            points = self.get_lidar_with_sweeps(index, self.max_sweeps, shift=shift)
        else:
            points = self.get_lidar_with_sweeps_host(index, self.max_sweeps)
            if shift is not None:
                points[:, 0:3] += shift
        data = {"points": points, "frame_id": Path(info["lidar_path"]).stem, "metadata": {"token": info["token"]}}
        if "gt_boxes" in info:
            min_points = self.dataset_cfg.get("FILTER_MIN_POINTS_IN_GT", False)
            keep = info["num_lidar_pts"] > min_points - 1 if min_points else slice(None)
            data["gt_names"], data["gt_boxes"] = info["gt_names"][keep], info["gt_boxes"][keep]
            if self.shift_coor:
                data["gt_boxes"][:, 0:3] += self.shift_coor
        return data

    def __getitem__(self, index):
        if self._merge_all_iters_to_one_epoch:
            index = index % len(self.infos)
        data = self.raw_frame(index)
        data = self.prepare_data(data)
        if "gt_boxes" in data:
            if self.dataset_cfg.get("SET_NAN_VELOCITY_TO_ZEROS", False):
                data["gt_boxes"][np.isnan(data["gt_boxes"])] = 0
            if not self.dataset_cfg.get("PRED_VELOCITY", False):
                data["gt_boxes"] = data["gt_boxes"][:, [0, 1, 2, 3, 4, 5, 6, -1]]
            if self.training and len(data["gt_boxes"]) == 0:            # reference dataset.py:152-154
                return self[np.random.randint(len(self))]
        return data

    # ---- predictions
    def generate_prediction_dicts(self, batch_dict, pred_dicts, class_names, output_path=None):
        """Per frame {name, score, boxes_lidar (SHIFT_COOR undone), pred_labels, frame_id, metadata}; a frame without
        detections keeps the zero-length float fields of the reference's template."""
        annos = []
        for index, box_dict in enumerate(pred_dicts):
            scores = box_dict["pred_scores"].detach().cpu().numpy()
            boxes = box_dict["pred_boxes"].detach().cpu().numpy()
            labels = box_dict["pred_labels"].detach().cpu().numpy()
            n = scores.shape[0]
            anno = {"name": np.zeros(n), "score": np.zeros(n), "boxes_lidar": np.zeros([n, 7]), "pred_labels": np.zeros(n)}
            if n:
                if self.shift_coor:
                    boxes[:, 0:3] -= self.shift_coor
                anno.update(name=np.array(class_names)[labels - 1], score=scores, boxes_lidar=boxes, pred_labels=labels)
            anno["frame_id"] = batch_dict["frame_id"][index]
            anno["metadata"] = batch_dict["metadata"][index]
            annos.append(anno)
        return annos

    def evaluation(self, det_annos, class_names, **kwargs):
        metric = kwargs.get("eval_metric", None)
        if metric == "kitti":
            return self.kitti_eval(copy.deepcopy(det_annos), copy.deepcopy(self.infos), class_names)
        if metric == "nuscenes":
            return self.nuscene_eval(det_annos, class_names, **kwargs)
        if metric == "nds":
            return self.nds_eval(det_annos, class_names, **kwargs)
        raise NotImplementedError(f"eval_metric '{metric}': NuScenesDataset scores with 'kitti', 'nds' (or 'nuscenes' through the nuScenes devkit)")

    def kitti_eval(self, eval_det_annos, eval_gt_annos, class_names):
        """The KITTI AP table in the LiDAR frame: detections and infos pair up by position, car / pedestrian / truck map to
        their KITTI names and every other class to Person_sitting, every object gets the placeholder image box (so all are
        Easy), and the LiDAR boxes become camera location / dimensions / rotation_y / alpha."""
        from ..kitti import kitti_utils
        from ..kitti.kitti_object_eval_python import eval as kitti_eval
        if (self.dataset_cfg.get("GT_FILTER", None) or {}).get("FOV_FILTER", None):
            raise NotImplementedError("GT_FILTER.FOV_FILTER: the reference calls an extract_fov_gt that it does not define; "
                                      "NuScenesDataset scores every ground-truth box")
        gt_annos = [{"name": np.array(info["gt_names"], dtype=object), "gt_boxes_lidar": np.asarray(info["gt_boxes"], np.float64)[:, :7].copy()}
                    for info in eval_gt_annos]
        for anno in eval_det_annos:
            anno["name"] = np.array(anno["name"], dtype=object)
            anno["boxes_lidar"] = np.asarray(anno["boxes_lidar"], np.float64)[:, :7]
        full = {}
        for anno in eval_det_annos + gt_annos:
            for name in anno["name"]:
                full[name] = MAP_NAME_TO_KITTI.get(name, "Person_sitting")
        kitti_utils.transform_annotations_to_kitti_format(eval_det_annos, map_name_to_kitti=full)
        kitti_utils.transform_annotations_to_kitti_format(gt_annos, map_name_to_kitti=full)
        kitti_class_names = [MAP_NAME_TO_KITTI.get(c, "Person_sitting") for c in class_names]
        return kitti_eval.get_official_eval_result(gt_annos, eval_det_annos, kitti_class_names)

    def nuscene_eval(self, det_annos, class_names, **kwargs):
        try:
            import nuscenes  # noqa: F401
        except ImportError as e:
            raise ImportError("eval_metric 'nuscenes' (NDS / mAP) runs the evaluator of the nuScenes devkit (package nuscenes-devkit, "
                              "module `nuscenes`), which is not installed; score with eval_metric 'kitti' instead") from e
        raise NotImplementedError("the nuScenes devkit evaluator is not wired up: score with eval_metric 'kitti'")

    def nds_eval(self, det_annos, class_names, **kwargs):
        """nuScenes mAP / NDS by the project's own evaluator (nuscenes_eval.py): results_nusc.json and metrics_summary.json under
        output_path, the reference's report text and {trans_err, ..., mAP, NDS}."""
        from . import nuscenes_eval
        if kwargs.get("output_path", None) is None:
            raise ValueError("eval_metric 'nds' writes results_nusc.json and metrics_summary.json: pass output_path")
        return nuscenes_eval.evaluate(self.infos, det_annos, self.class_names if self.class_names else class_names, self.root_path,
                                      self.dataset_cfg.VERSION, kwargs["output_path"], logger=self.logger)

    # ---- GT database: the frames through augmentor/database_sampler.create_groundtruth_database
    def create_groundtruth_database(self, used_classes=None, max_sweeps=10):
        from ..augmentor.database_sampler import create_groundtruth_database
        return create_groundtruth_database(_InfoFrames(self, max_sweeps), self.root_path, used_classes=used_classes, packed=False,
                                           db_name=f"gt_database_{max_sweeps}sweeps_withvelo",
                                           info_name=f"nuscenes_dbinfos_{max_sweeps}sweeps_withvelo.pkl")


class _InfoFrames:
    """The dataset's frames as database_sampler.create_groundtruth_database reads a dataset: len() and raw_sample(k) ->
    (merged points [n, 5] numpy, gt_boxes [m, 9], gt_names)."""

    def __init__(self, dataset, max_sweeps):
        self.dataset, self.max_sweeps = dataset, max_sweeps

    def __len__(self):
        return len(self.dataset.infos)

    def raw_sample(self, k):
        info = self.dataset.infos[k]
        if self.max_sweeps > 1:
            points = self.dataset.get_lidar_with_sweeps(k, self.max_sweeps).cpu().numpy()
        else:
            points = self.dataset.get_lidar_with_sweeps_host(k, 1)
        return points, info["gt_boxes"], info["gt_names"]


def main(argv=None):
    import argparse

    from ...config import AttrDict, cfg_from_yaml_file
    ap = argparse.ArgumentParser()
    ap.add_argument("command", choices=["create_nuscenes_gt_database", "create_nuscenes_infos"])
    ap.add_argument("cfg_file", help="dataset yaml, e.g. toda_amd/tools/cfgs/dataset_configs/nuscenes_dataset.yaml")
    ap.add_argument("--data_path", default=None, help="nuScenes root (the directory that holds <VERSION>); default: DATA_PATH of the yaml")
    ap.add_argument("--version", default=None, help="default: VERSION of the yaml")
    args = ap.parse_args(argv)
    if args.command == "create_nuscenes_infos":
        raise SystemExit("create_nuscenes_infos is out of scope: the info builder walks the nuScenes devkit's tables.  Prepare "
                         "nuscenes_infos_10sweeps_{train,val}.pkl with a stock OpenPCDet installation; they are read as they are, and "
                         "create_nuscenes_gt_database builds the GT-sampling database from them.")
    dataset_cfg = cfg_from_yaml_file(args.cfg_file, AttrDict())
    if args.version:
        dataset_cfg.VERSION = args.version
    dataset_cfg.pop("DATA_AUGMENTOR", None)          # the sampler would look for the database that is being built
    dataset_cfg.BALANCED_RESAMPLING = False
    dataset = NuScenesDataset(dataset_cfg, class_names=[], root_path=Path(args.data_path or dataset_cfg.DATA_PATH), training=True)
    db = dataset.create_groundtruth_database(max_sweeps=int(dataset_cfg.MAX_SWEEPS))
    for name, entries in db.items():
        print("Database %s: %d" % (name, len(entries)))


if __name__ == "__main__":
    main()
