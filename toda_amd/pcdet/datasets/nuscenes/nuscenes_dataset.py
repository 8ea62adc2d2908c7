"""NuScenesDataset (behaviour of reference pcdet/datasets/nuscenes/nuscenes_dataset.py): the nuScenes LiDAR sweeps on disk and
the info pickles of a stock OpenPCDet preparation -> training / evaluation samples, the GT-sampling database, prediction dicts
and the KITTI-style AP.

    <DATA_PATH>/<VERSION>/{samples,sweeps}/LIDAR_TOP/*.pcd.bin          [-1, 5] fp32: x, y, z, intensity, ring
    <DATA_PATH>/<VERSION>/nuscenes_infos_10sweeps_{train,val}.pkl       list of {lidar_path, token, sweeps[{lidar_path,
                                                                        transform_matrix, time_lag, ...}], gt_boxes [n, 9],
                                                                        gt_names, num_lidar_pts, ...}

The reading, the merge on the device and the numpy route are SweepDataset's (sweep_dataset.py).  Here: the square ego cut,
SHIFT_COOR, class-balanced resampling, FILTER_MIN_POINTS_IN_GT, the velocity columns and the nuScenes metrics.

Out of scope, because they walk the nuScenes devkit's tables: the info builder (create_nuscenes_infos) and the devkit's own
evaluator (eval_metric 'nuscenes' raises ImportError without the devkit).  eval_metric 'kitti' is served, and eval_metric 'nds'
is the nuScenes mAP / NDS by the project's evaluator (nuscenes_eval.py, matching on the device).

    python -m toda_amd.pcdet.datasets.nuscenes.nuscenes_dataset create_nuscenes_gt_database <dataset yaml> [--data_path DIR] [--version V]
"""
import numpy as np

from .. import sweep_dataset
from ..dataset import lidar_prediction_dicts
from ..sweep_dataset import ROW_BYTES, SweepDataset  # noqa: F401  (ROW_BYTES stays importable from here)

MAP_NAME_TO_KITTI = {"car": "Car", "pedestrian": "Pedestrian", "truck": "Truck"}
EGO_RADIUS = 1.0                 # half side of the square around the sensor that holds the ego vehicle's own returns


class NuScenesDataset(SweepDataset):
    NAME = "NuScenes"
    EGO_HALF_SIDES = (EGO_RADIUS, EGO_RADIUS)

    def __init__(self, dataset_cfg, class_names, training=True, root_path=None, logger=None):
        super().__init__(dataset_cfg=dataset_cfg, class_names=class_names, training=training, root_path=root_path, logger=logger)
        self.shift_coor = dataset_cfg.get("SHIFT_COOR", None)
        self.include_nuscenes_data(self.mode)
        if self.training and dataset_cfg.get("BALANCED_RESAMPLING", False):
            self.infos = self.balanced_infos_resampling(self.infos)

    def include_nuscenes_data(self, mode):
        self.include_infos(mode)

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

    # ---- samples
    def raw_frame(self, index):
        """Sample `index` before prepare_data: {points (SHIFT_COOR added), frame_id, metadata} and, with annotations, gt_boxes
        [n, 9] / gt_names (FILTER_MIN_POINTS_IN_GT applied, SHIFT_COOR added)."""
        data = super().raw_frame(index, shift=np.array(self.shift_coor, dtype=np.float32) if self.shift_coor else None)
        if "gt_boxes" in data:
            min_points = self.dataset_cfg.get("FILTER_MIN_POINTS_IN_GT", False)
            keep = self.infos[index]["num_lidar_pts"] > min_points - 1 if min_points else slice(None)
            data["gt_names"], data["gt_boxes"] = data["gt_names"][keep], data["gt_boxes"][keep]
            if self.shift_coor:
                data["gt_boxes"][:, 0:3] += self.shift_coor
        return data

    def finish_sample(self, data):
        if "gt_boxes" in data:
            if self.dataset_cfg.get("SET_NAN_VELOCITY_TO_ZEROS", False):
                data["gt_boxes"][np.isnan(data["gt_boxes"])] = 0
            if not self.dataset_cfg.get("PRED_VELOCITY", False):
                data["gt_boxes"] = data["gt_boxes"][:, [0, 1, 2, 3, 4, 5, 6, -1]]
        return data

    # ---- predictions
    def generate_prediction_dicts(self, batch_dict, pred_dicts, class_names, output_path=None):
        """SweepDataset's record with SHIFT_COOR undone on boxes_lidar."""
        return lidar_prediction_dicts(batch_dict, pred_dicts, class_names, shift=self.shift_coor)

    def own_metric(self, metric, det_annos, class_names, **kwargs):
        if metric == "nuscenes":
            return self.nuscene_eval(det_annos, class_names, **kwargs)
        if metric == "nds":
            return self.nds_eval(det_annos, class_names, **kwargs)
        raise NotImplementedError(f"eval_metric '{metric}': NuScenesDataset scores with 'kitti', 'nds' (or 'nuscenes' through the nuScenes devkit)")

    def kitti_eval(self, eval_det_annos, eval_gt_annos, class_names):
        """SweepDataset.lidar_kitti_table of every ground-truth box: car / pedestrian / truck map to their KITTI names and every
        other class, evaluated or not, to Person_sitting."""
        if (self.dataset_cfg.get("GT_FILTER", None) or {}).get("FOV_FILTER", None):
            raise NotImplementedError("GT_FILTER.FOV_FILTER: the reference calls an extract_fov_gt that it does not define; "
                                      "NuScenesDataset scores every ground-truth box")
        gt_annos = [{"name": info["gt_names"], "gt_boxes_lidar": np.asarray(info["gt_boxes"], np.float64)[:, :7].copy()} for info in eval_gt_annos]
        return self.lidar_kitti_table(eval_det_annos, gt_annos, MAP_NAME_TO_KITTI, [MAP_NAME_TO_KITTI.get(c, "Person_sitting") for c in class_names])

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

    def create_groundtruth_database(self, used_classes=None, max_sweeps=10):
        return self.write_groundtruth_database(used_classes, max_sweeps, f"gt_database_{max_sweeps}sweeps_withvelo",
                                               f"nuscenes_dbinfos_{max_sweeps}sweeps_withvelo.pkl")


def main(argv=None):
    sweep_dataset.main(NuScenesDataset, "create_nuscenes_gt_database", "create_nuscenes_infos",
                       "create_nuscenes_infos is out of scope: the info builder walks the nuScenes devkit's tables.  Prepare "
                       "nuscenes_infos_10sweeps_{train,val}.pkl with a stock OpenPCDet installation; they are read as they are, and "
                       "create_nuscenes_gt_database builds the GT-sampling database from them.", argv, overrides=[("BALANCED_RESAMPLING", False)])


if __name__ == "__main__":
    main()
