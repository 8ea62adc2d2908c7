"""SweepDataset: what the datasets of multi-sweep LiDAR samples (NuScenesDataset, LyftDataset) share.  A sample is a key frame
and MAX_SWEEPS - 1 earlier sweeps, each a file of [-1, 5] fp32 rows (x, y, z, intensity, ring), listed by the info pickles of a
stock OpenPCDet preparation under <DATA_PATH>/<VERSION>.  A subclass states, as class attributes, its name in the log, the
half-sides of the ego rectangle and what happens to a file that is no whole number of rows.

MI355X layout: the files are read into one host buffer, go to the device in one H2D copy, and one kernel pass
(ops.sweeps_merge_rect, csrc/nuscenes_frame.hip) flags the ego vehicle's points in the sweeps (never in the key frame), moves
every sweep into the key frame (fp64 product, one rounding to fp32), adds the shift and stamps the time lag; the stable
compaction (ops.RowBuffer) drops the flagged rows, and the range mask, the shuffle and the voxeliser of the data processor follow
on the device.  The reference does this per sweep in numpy inside DataLoader workers.  With MAX_SWEEPS > 1 the samples are CUDA
tensors (`on_device`): build_dataloader then runs the dataset in the training process, no worker process opens the GPU.  With
MAX_SWEEPS == 1 there is nothing to merge: the key frame stays numpy and reaches the device with the batch.
get_lidar_with_sweeps_host is the same work in the reference's numpy arithmetic: the test oracle and the bench baseline."""
import copy
import os
import pickle
from pathlib import Path

import numpy as np
import torch

from .dataset import DatasetTemplate, lidar_kitti_eval, lidar_prediction_dicts

ROW_BYTES = 20                   # x, y, z, intensity, ring as fp32


class SweepDataset(DatasetTemplate):
    NAME = None                  # the dataset in the log lines and in the command line's help
    EGO_HALF_SIDES = None        # (x, y) half-sides of the rectangle around the sensor that holds the ego vehicle's own returns
    DROP_FILE_TAIL = False       # a file that is no whole number of rows: refused (False) or read up to its last whole row (True)

    def __init__(self, dataset_cfg, class_names, training=True, root_path=None, logger=None):
        root_path = Path(root_path if root_path is not None else dataset_cfg.DATA_PATH) / dataset_cfg.VERSION
        super().__init__(dataset_cfg=dataset_cfg, class_names=class_names, training=training, root_path=root_path, logger=logger)
        self.max_sweeps = int(dataset_cfg.get("MAX_SWEEPS", 1))
        # samples leave __getitem__ as CUDA tensors: build_dataloader keeps such a dataset in the training process
        self.on_device = self.max_sweeps > 1
        self.infos = []

    # ---- reading
    def include_infos(self, mode):
        self._log("Loading %s dataset" % self.NAME)
        for rel in self.dataset_cfg.INFO_PATH[mode]:
            path = self.root_path / rel
            if not path.exists():
                continue
            with open(path, "rb") as f:
                self.infos.extend(pickle.load(f))
        interval = int((self.dataset_cfg.get("SAMPLED_INTERVAL", None) or {}).get(mode, 1))
        if interval > 1:
            self.infos = self.infos[::interval]
        self._log("Total samples for %s dataset: %d" % (self.NAME, len(self.infos)))

    def _sweep_table(self, info, max_sweeps):
        """The files of a sample, key frame first, then max_sweeps - 1 of the info's sweeps in the order np.random.choice
        draws them: (paths, matrices, time lags, drop-ego flags).  The key frame is never cut."""
        picks = np.random.choice(len(info["sweeps"]), max_sweeps - 1, replace=False)
        sweeps = [info["sweeps"][k] for k in picks]
        return ([self.root_path / info["lidar_path"]] + [self.root_path / s["lidar_path"] for s in sweeps],
                [None] + [s["transform_matrix"] for s in sweeps], [0.0] + [s["time_lag"] for s in sweeps], [False] + [True] * len(sweeps))

    @classmethod
    def read_rows(cls, paths):
        """The whole rows of the files in one host buffer: ([n, 5] fp32, row offsets per file).  With DROP_FILE_TAIL the bytes
        past a file's last whole row are not read (reference lyft_dataset.py:44-46)."""
        counts = []
        for path in paths:
            size = os.path.getsize(path)
            if size % ROW_BYTES and not cls.DROP_FILE_TAIL:
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

    def merge_info(self, info, max_sweeps, shift=None):
        """[n, 5] CUDA tensor (x, y, z, intensity, time lag) of one info: the key frame, then the drawn sweeps without the ego
        vehicle's points, in the key frame's coordinates, `shift` added.  One upload, one kernel pass, one compaction."""
        from ... import ops
        paths, matrices, lags, drop_ego = self._sweep_table(info, max_sweeps)
        rows, offsets = self.read_rows(paths)
        dev = torch.from_numpy(rows).cuda()
        out, flags = ops.sweeps_merge_rect(dev, offsets, matrices, lags, drop_ego, *self.EGO_HALF_SIDES, shift=shift)
        return ops.RowBuffer(out.shape[0], 5, out.device).append(out, flags, 1).finish()

    def get_lidar_with_sweeps(self, index, max_sweeps=1, shift=None):
        """merge_info of sample `index`."""
        return self.merge_info(self.infos[index], max_sweeps, shift=shift)

    @classmethod
    def read_points_host(cls, path):
        """[n, 4] fp32 view (x, y, z, intensity) of a file's rows; with DROP_FILE_TAIL the floats past the last whole row are
        dropped, without it the reshape refuses them."""
        raw = np.fromfile(str(path), dtype=np.float32)
        if cls.DROP_FILE_TAIL:
            raw = raw[:raw.size // 5 * 5]
        return raw.reshape(-1, 5)[:, :4]

    @classmethod
    def get_sweep_host(cls, path, matrix, time_lag):
        """One earlier sweep in numpy, the reference's arithmetic: ego cut on the raw coordinates, float64 product with the
        homogeneous points assigned into the fp32 cloud, a float64 time column."""
        pts = cls.read_points_host(path)
        pts = pts[~((np.abs(pts[:, 0]) < cls.EGO_HALF_SIDES[0]) & (np.abs(pts[:, 1]) < cls.EGO_HALF_SIDES[1]))]
        if matrix is not None:
            hom = np.concatenate([pts[:, :3].T, np.ones((1, pts.shape[0]))], axis=0)
            pts[:, :3] = np.asarray(matrix).dot(hom)[:3].T
        return pts, np.full((pts.shape[0], 1), time_lag, dtype=np.float64)

    def get_lidar_with_sweeps_host(self, index, max_sweeps=1):
        """get_lidar_with_sweeps in numpy without the shift (the reference's route): [n, 5] fp32."""
        paths, matrices, lags, _ = self._sweep_table(self.infos[index], max_sweeps)
        key = self.read_points_host(paths[0])
        clouds, times = [key], [np.zeros((key.shape[0], 1))]
        for path, matrix, lag in zip(paths[1:], matrices[1:], lags[1:]):
            pts, stamp = self.get_sweep_host(path, matrix, lag)
            clouds.append(pts)
            times.append(stamp)
        points = np.concatenate(clouds, axis=0)
        return np.concatenate([points, np.concatenate(times, axis=0).astype(points.dtype)], axis=1)

    # ---- samples
    def raw_frame(self, index, shift=None):
        """Sample `index` before prepare_data: {points (`shift` added), frame_id, metadata} and, with annotations, gt_boxes /
        gt_names as the info has them."""
        info = copy.deepcopy(self.infos[index])
        if self.on_device:
            points = self.get_lidar_with_sweeps(index, self.max_sweeps, shift=shift)
        else:
            points = self.get_lidar_with_sweeps_host(index, self.max_sweeps)
            if shift is not None:
                points[:, 0:3] += shift
        data = {"points": points, "frame_id": Path(info["lidar_path"]).stem, "metadata": {"token": info["token"]}}
        if "gt_boxes" in info:
            data["gt_boxes"], data["gt_names"] = info["gt_boxes"], info["gt_names"]
        return data

    def finish_sample(self, data):
        """What a subclass does to a sample after prepare_data; nothing here."""
        return data

    def __getitem__(self, index):
        if self._merge_all_iters_to_one_epoch:
            index = index % len(self.infos)
        data = self.finish_sample(self.prepare_data(self.raw_frame(index)))
        if self.training and "gt_boxes" in data and len(data["gt_boxes"]) == 0:            # reference dataset.py:152-154
            return self[np.random.randint(len(self))]
        return data

    # ---- predictions
    def generate_prediction_dicts(self, batch_dict, pred_dicts, class_names, output_path=None):
        return lidar_prediction_dicts(batch_dict, pred_dicts, class_names)

    def evaluation(self, det_annos, class_names, **kwargs):
        """eval_metric 'kitti' through the subclass's kitti_eval on copies of the detections and the infos; every other metric is
        the subclass's own (own_metric)."""
        metric = kwargs.get("eval_metric", None)
        if metric == "kitti":
            return self.kitti_eval(copy.deepcopy(det_annos), copy.deepcopy(self.infos), class_names)
        return self.own_metric(metric, det_annos, class_names, **kwargs)

    def lidar_kitti_table(self, det_annos, gt_annos, map_name_to_kitti, kitti_class_names, info_with_fakelidar=False):
        """The KITTI AP table in the LiDAR frame: detections and ground truth pair up by position, the objects of a class that
        map_name_to_kitti does not name count as Person_sitting, and every object gets the placeholder image box (so all are
        Easy)."""
        full = {}
        for anno in det_annos + gt_annos:
            for name in anno["name"]:
                full[name] = map_name_to_kitti.get(name, "Person_sitting")
        return lidar_kitti_eval(det_annos, gt_annos, full, kitti_class_names, info_with_fakelidar)

    # ---- GT database: the frames through augmentor/database_sampler.create_groundtruth_database
    def write_groundtruth_database(self, used_classes, max_sweeps, db_name, info_name):
        from .augmentor.database_sampler import create_groundtruth_database
        return create_groundtruth_database(_InfoFrames(self, max_sweeps), self.root_path, used_classes=used_classes, packed=False,
                                           db_name=db_name, info_name=info_name)


class _InfoFrames:
    """The dataset's frames as database_sampler.create_groundtruth_database reads a dataset: len() and raw_sample(k) ->
    (merged points [n, 5] numpy, gt_boxes as the info has them, gt_names)."""

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


def main(cls, gt_command, info_command, out_of_scope, argv=None, overrides=()):
    """The command line of a sweep dataset's module: `gt_command` builds the GT-sampling database of `cls` from the infos,
    `info_command` exits with `out_of_scope`.  overrides: (key, value) pairs set in the yaml before the dataset is built."""
    import argparse

    from ..config import AttrDict, cfg_from_yaml_file
    ap = argparse.ArgumentParser()
    ap.add_argument("command", choices=[gt_command, info_command])
    ap.add_argument("cfg_file", help=f"dataset yaml, e.g. toda_amd/tools/cfgs/dataset_configs/{cls.NAME.lower()}_dataset.yaml")
    ap.add_argument("--data_path", default=None, help=f"{cls.NAME} root (the directory that holds <VERSION>); default: DATA_PATH of the yaml")
    ap.add_argument("--version", default=None, help="default: VERSION of the yaml")
    args = ap.parse_args(argv)
    if args.command == info_command:
        raise SystemExit(out_of_scope)
    dataset_cfg = cfg_from_yaml_file(args.cfg_file, AttrDict())
    if args.version:
        dataset_cfg.VERSION = args.version
    dataset_cfg.pop("DATA_AUGMENTOR", None)          # the sampler would look for the database that is being built
    for key, value in overrides:
        dataset_cfg[key] = value
    dataset = cls(dataset_cfg, class_names=[], root_path=Path(args.data_path or dataset_cfg.DATA_PATH), training=True)
    db = dataset.create_groundtruth_database(max_sweeps=int(dataset_cfg.MAX_SWEEPS))
    for name, entries in db.items():
        print("Database %s: %d" % (name, len(entries)))
