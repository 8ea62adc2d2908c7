"""LyftDataset (behaviour of reference pcdet/datasets/lyft/lyft_dataset.py): the Lyft Level 5 LiDAR sweeps on disk and the info
pickles of a stock OpenPCDet preparation -> training / evaluation samples, the GT-sampling database, prediction dicts, the
KITTI-style AP and the Lyft mAP.

    <DATA_PATH>/<VERSION>/<lidar_path of the infos>                     [-1, 5] fp32: x, y, z, intensity, ring
    <DATA_PATH>/<VERSION>/lyft_infos_{train,val}.pkl                    list of {lidar_path, token, ref_to_car, car_to_global,
                                                                        sweeps[{lidar_path, transform_matrix, time_lag, ...}],
                                                                        gt_boxes [n, 7], gt_names, ...}
    <DATA_PATH>/<VERSION>/data/{sample_annotation,instance,category}.json   read by eval_metric 'lyft' only

nuScenes-like, but not equal to it: MAX_SWEEPS is 5; the ego cut is a rectangle of 1.5 m x 1.0 m half-sides and applies to the
sweeps only, never to the key frame; boxes have 7 columns (no velocity); a file whose size is no whole number of 20-byte rows
loses its tail instead of being refused (the Lyft set holds a few such files).

MI355X layout, as NuScenesDataset: the files are read into one host buffer, go to the device in one H2D copy, one kernel pass
(ops.sweeps_merge_rect, csrc/nuscenes_frame.hip) flags the ego vehicle's points, moves every sweep into the key frame (fp64
product, one rounding to fp32) and stamps the time lag, and the stable compaction (ops.RowBuffer) drops the flagged rows.  With
MAX_SWEEPS > 1 the samples are CUDA tensors (`on_device`): build_dataloader then runs the dataset in the training process.
get_lidar_with_sweeps_host is the same work in the reference's numpy arithmetic: the test oracle and the bench baseline.

Out of scope, because it walks the Lyft SDK's tables: the info builder (create_lyft_infos).  eval_metric 'kitti' is served by the
project's KITTI evaluator, eval_metric 'lyft' by the project's own evaluator (lyft_eval.py, IoU and matching on the device).

    python -m toda_amd.pcdet.datasets.lyft.lyft_dataset create_lyft_gt_database <dataset yaml> [--data_path DIR] [--version V]
"""
import copy
import os
import pickle
from pathlib import Path

import numpy as np
import torch

from ..dataset import DatasetTemplate

MAP_NAME_TO_KITTI = {"car": "Car", "pedestrian": "Pedestrian", "truck": "Truck", "bicycle": "Cyclist", "motorcycle": "Cyclist"}
EGO_RADIUS_X, EGO_RADIUS_Y = 1.5, 1.0       # half-sides of the rectangle around the sensor that holds the ego vehicle's own returns
ROW_BYTES = 20                              # x, y, z, intensity, ring as fp32


class LyftDataset(DatasetTemplate):
    def __init__(self, dataset_cfg, class_names, training=True, root_path=None, logger=None):
        root_path = Path(root_path if root_path is not None else dataset_cfg.DATA_PATH) / dataset_cfg.VERSION
        super().__init__(dataset_cfg=dataset_cfg, class_names=class_names, training=training, root_path=root_path, logger=logger)
        self.max_sweeps = int(dataset_cfg.get("MAX_SWEEPS", 1))
        # samples leave __getitem__ as CUDA tensors: build_dataloader keeps such a dataset in the training process
        self.on_device = self.max_sweeps > 1
        self.infos = []
        self.include_lyft_data(self.mode)

    def _log(self, text):
        if self.logger is not None:
            self.logger.info(text)

    # ---- reading
    def include_lyft_data(self, mode):
        self._log("Loading lyft dataset")
        for rel in self.dataset_cfg.INFO_PATH[mode]:
            path = self.root_path / rel
            if not path.exists():
                continue
            with open(path, "rb") as f:
                self.infos.extend(pickle.load(f))
        self._log("Total samples for lyft dataset: %d" % len(self.infos))

    def _sweep_table(self, info, max_sweeps):
        """The files of a sample, key frame first, then max_sweeps - 1 of the info's sweeps in the order np.random.choice
        draws them: (paths, matrices, time lags, drop-ego flags).  The key frame is never cut."""
        picks = np.random.choice(len(info["sweeps"]), max_sweeps - 1, replace=False)
        sweeps = [info["sweeps"][k] for k in picks]
        return ([self.root_path / info["lidar_path"]] + [self.root_path / s["lidar_path"] for s in sweeps],
                [None] + [s["transform_matrix"] for s in sweeps], [0.0] + [s["time_lag"] for s in sweeps], [False] + [True] * len(sweeps))

    @staticmethod
    def read_rows(paths):
        """The whole rows of the files in one host buffer: ([n, 5] fp32, row offsets per file).  Bytes past a file's last whole
        row are not read (reference lyft_dataset.py:44-46)."""
        counts = [os.path.getsize(path) // ROW_BYTES for path in paths]
        offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        rows = np.empty((int(offsets[-1]), 5), np.float32)
        for path, lo, hi in zip(paths, offsets[:-1], offsets[1:]):
            if hi > lo:
                with open(path, "rb") as f:
                    got = f.readinto(memoryview(rows[lo:hi]).cast("B"))
                if got != (hi - lo) * ROW_BYTES:
                    raise ValueError(f"{path}: short read")
        return rows, [int(o) for o in offsets]

    def get_lidar_with_sweeps(self, index, max_sweeps=1):
        """[n, 5] CUDA tensor (x, y, z, intensity, time lag): the key frame, then the drawn sweeps without the ego vehicle's
        points, in the key frame's coordinates.  One upload, one kernel pass, one compaction."""
        from .... import ops
        paths, matrices, lags, drop_ego = self._sweep_table(self.infos[index], max_sweeps)
        rows, offsets = self.read_rows(paths)
        dev = torch.from_numpy(rows).cuda()
        out, flags = ops.sweeps_merge_rect(dev, offsets, matrices, lags, drop_ego, EGO_RADIUS_X, EGO_RADIUS_Y)
        return ops.RowBuffer(out.shape[0], 5, out.device).append(out, flags, 1).finish()

    @staticmethod
    def read_points_host(path):
        """[n, 4] fp32 view (x, y, z, intensity) of a file's whole rows; floats past the last whole row are dropped."""
        raw = np.fromfile(str(path), dtype=np.float32)
        return raw[:raw.size // 5 * 5].reshape(-1, 5)[:, :4]

    @classmethod
    def get_sweep_host(cls, path, matrix, time_lag):
        """One earlier sweep in numpy, the reference's arithmetic: ego cut on the raw coordinates, float64 product with the
        homogeneous points assigned into the fp32 cloud, a float64 time column."""
        pts = cls.read_points_host(path)
        pts = pts[~((np.abs(pts[:, 0]) < EGO_RADIUS_X) & (np.abs(pts[:, 1]) < EGO_RADIUS_Y))]
        if matrix is not None:
            hom = np.concatenate([pts[:, :3].T, np.ones((1, pts.shape[0]))], axis=0)
            pts[:, :3] = np.asarray(matrix).dot(hom)[:3].T
        return pts, np.full((pts.shape[0], 1), time_lag, dtype=np.float64)

    def get_lidar_with_sweeps_host(self, index, max_sweeps=1):
        """get_lidar_with_sweeps in numpy (the reference's route): [n, 5] fp32."""
        paths, matrices, lags, _ = self._sweep_table(self.infos[index], max_sweeps)
        key = self.read_points_host(paths[0])
        clouds, times = [key], [np.zeros((key.shape[0], 1))]
        for path, matrix, lag in zip(paths[1:], matrices[1:], lags[1:]):
            pts, stamp = self.get_sweep_host(path, matrix, lag)
            clouds.append(pts)
            times.append(stamp)
        points = np.concatenate(clouds, axis=0)
        return np.concatenate((points, np.concatenate(times, axis=0).astype(points.dtype)), axis=1)

    # ---- samples
    def __len__(self):
        if self._merge_all_iters_to_one_epoch:
            return len(self.infos) * self.total_epochs
        return len(self.infos)

    def raw_frame(self, index):
        """Sample `index` before prepare_data: {points, frame_id, metadata} and, with annotations, gt_names / gt_boxes [n, 7]."""
        info = copy.deepcopy(self.infos[index])
        if self.on_device:
            points = self.get_lidar_with_sweeps(index, self.max_sweeps)
        else:
            points = self.get_lidar_with_sweeps_host(index, self.max_sweeps)
        data = {"points": points, "frame_id": Path(info["lidar_path"]).stem, "metadata": {"token": info["token"]}}
        if "gt_boxes" in info:
            data["gt_boxes"], data["gt_names"] = info["gt_boxes"], info["gt_names"]
        return data

    def __getitem__(self, index):
        if self._merge_all_iters_to_one_epoch:
            index = index % len(self.infos)
        data = self.prepare_data(self.raw_frame(index))
        if "gt_boxes" in data and self.training and len(data["gt_boxes"]) == 0:            # reference dataset.py:152-154
            return self[np.random.randint(len(self))]
        return data

    # ---- predictions
    def generate_prediction_dicts(self, batch_dict, pred_dicts, class_names, output_path=None):
        """Per frame {name, score, boxes_lidar, pred_labels, frame_id, metadata}; a frame without detections keeps the
        zero-length float fields of the reference's template."""
        annos = []
        for index, box_dict in enumerate(pred_dicts):
            scores = box_dict["pred_scores"].detach().cpu().numpy()
            boxes = box_dict["pred_boxes"].detach().cpu().numpy()
            labels = box_dict["pred_labels"].detach().cpu().numpy()
            n = scores.shape[0]
            anno = {"name": np.zeros(n), "score": np.zeros(n), "boxes_lidar": np.zeros([n, 7]), "pred_labels": np.zeros(n)}
            if n:
                anno.update(name=np.array(class_names)[labels - 1], score=scores, boxes_lidar=boxes, pred_labels=labels)
            anno["frame_id"] = batch_dict["frame_id"][index]
            anno["metadata"] = batch_dict["metadata"][index]
            annos.append(anno)
        return annos

    def evaluation(self, det_annos, class_names, **kwargs):
        metric = kwargs.get("eval_metric", None)
        if metric == "kitti":
            return self.kitti_eval(copy.deepcopy(det_annos), copy.deepcopy(self.infos), class_names)
        if metric == "lyft":
            return self.lyft_eval(det_annos, class_names, iou_thresholds=self.dataset_cfg.EVAL_LYFT_IOU_LIST)
        raise NotImplementedError(f"eval_metric '{metric}': LyftDataset scores with 'kitti' or 'lyft'")

    def kitti_eval(self, eval_det_annos, eval_gt_annos, class_names):
        """The KITTI AP table in the LiDAR frame: detections and infos pair up by position; car, pedestrian, truck, bicycle and
        motorcycle map to their KITTI names (the reference's map).  Every evaluated class must be in the map: another one
        raises the KeyError that names it.  Objects of other classes among the boxes count as Person_sitting, as
        NuScenesDataset counts them, and every object gets the placeholder image box (so all are Easy)."""
        from ..kitti import kitti_utils
        from ..kitti.kitti_object_eval_python import eval as kitti_eval
        for name in class_names:
            if name not in MAP_NAME_TO_KITTI:
                raise KeyError(f"'{name}': eval_metric 'kitti' of LyftDataset maps {sorted(MAP_NAME_TO_KITTI)} only; score the other "
                               "classes with eval_metric 'lyft'")
        gt_annos = [{"name": np.array(info["gt_names"], dtype=object), "gt_boxes_lidar": np.asarray(info["gt_boxes"], np.float64).reshape(-1, 7).copy()}
                    for info in eval_gt_annos]
        for anno in eval_det_annos:
            anno["name"] = np.array(anno["name"], dtype=object)
            anno["boxes_lidar"] = np.asarray(anno["boxes_lidar"], np.float64)[:, :7]
        full = {}
        for anno in eval_det_annos + gt_annos:
            for name in anno["name"]:
                full[name] = MAP_NAME_TO_KITTI.get(name, "Person_sitting")
        fake = bool(self.dataset_cfg.get("INFO_WITH_FAKELIDAR", False))
        kitti_utils.transform_annotations_to_kitti_format(eval_det_annos, map_name_to_kitti=full)
        kitti_utils.transform_annotations_to_kitti_format(gt_annos, map_name_to_kitti=full, info_with_fakelidar=fake)
        return kitti_eval.get_official_eval_result(gt_annos, eval_det_annos, [MAP_NAME_TO_KITTI[c] for c in class_names])

    def lyft_eval(self, det_annos, class_names, iou_thresholds=(0.5,)):
        """The Lyft mAP by the project's own evaluator (lyft_eval.py): the reference's report text and {class: AP, mAP}."""
        from . import lyft_eval
        return lyft_eval.evaluate(self.infos, det_annos, class_names, self.root_path, iou_thresholds, version=self.dataset_cfg.VERSION)

    # ---- GT database: the frames through augmentor/database_sampler.create_groundtruth_database
    def create_groundtruth_database(self, used_classes=None, max_sweeps=5):
        from ..augmentor.database_sampler import create_groundtruth_database
        return create_groundtruth_database(_InfoFrames(self, max_sweeps), self.root_path, used_classes=used_classes, packed=False,
                                           db_name="gt_database", info_name=f"lyft_dbinfos_{max_sweeps}sweeps.pkl")


class _InfoFrames:
    """The dataset's frames as database_sampler.create_groundtruth_database reads a dataset: len() and raw_sample(k) ->
    (merged points [n, 5] numpy, gt_boxes [m, 7], gt_names)."""

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


def create_lyft_info(*args, **kwargs):
    raise SystemExit("create_lyft_infos is out of scope: the info builder walks the Lyft SDK's tables (lyft_dataset_sdk).  Prepare "
                     "lyft_infos_{train,val}.pkl with a stock OpenPCDet installation; they are read as they are, and "
                     "create_lyft_gt_database builds the GT-sampling database from them.")


def main(argv=None):
    import argparse

    from ...config import AttrDict, cfg_from_yaml_file
    ap = argparse.ArgumentParser()
    ap.add_argument("command", choices=["create_lyft_gt_database", "create_lyft_infos"])
    ap.add_argument("cfg_file", help="dataset yaml, e.g. toda_amd/tools/cfgs/dataset_configs/lyft_dataset.yaml")
    ap.add_argument("--data_path", default=None, help="Lyft root (the directory that holds <VERSION>); default: DATA_PATH of the yaml")
    ap.add_argument("--version", default=None, help="default: VERSION of the yaml")
    args = ap.parse_args(argv)
    if args.command == "create_lyft_infos":
        create_lyft_info()
    dataset_cfg = cfg_from_yaml_file(args.cfg_file, AttrDict())
    if args.version:
        dataset_cfg.VERSION = args.version
    dataset_cfg.pop("DATA_AUGMENTOR", None)          # the sampler would look for the database that is being built
    dataset = LyftDataset(dataset_cfg, class_names=[], root_path=Path(args.data_path or dataset_cfg.DATA_PATH), training=True)
    db = dataset.create_groundtruth_database(max_sweeps=int(dataset_cfg.MAX_SWEEPS))
    for name, entries in db.items():
        print("Database %s: %d" % (name, len(entries)))


if __name__ == "__main__":
    main()
