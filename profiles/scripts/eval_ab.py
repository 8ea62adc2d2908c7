"""Do two trees (or two builds of libtoda_hip.so) compute the same bits in the KITTI, nuScenes and Waymo evaluators?

  python profiles/scripts/eval_ab.py dump DIR              every output of the cases below as DIR/<case>.<call>.<entry point>.<k>.npy
  python profiles/scripts/eval_ab.py compare DIR_A DIR_B   two such directories, array by array

`dump` runs the tree this file lies in (and the library TODA_HIP_LIB names, if set), so the parent's side is this file copied into a
worktree of the parent commit.  Every call of the seven entry points (eval_overlaps, eval_match_scores, eval_match, nusc_eval_prepare,
nusc_eval_match, waymo_eval_iou, waymo_eval_match) is recorded while the cases run; waymo_eval_match always runs with debug=True, so
the match table, which is what a changed tie rule would move, is among the outputs.  Of eval_match_scores only the entries the kernel
writes are kept (the first counts[f] of every frame).  `compare` asks for equal dtype, shape and bytes, which is numpy.array_equal
and NaN for NaN on top.  Exit status 1 when anything differs.

Cases (seeded, from tests/kitti_eval_cases.py, tests/nusc_eval_cases.py, tests/waymo_eval_cases.py and the edge grids of the GPU tests):
  kitti      40 mixed frames through get_official_eval_result; 3 frames with 64 < detections, one > 256, classes Car and Van
  nusc       the 6 x 6 size grid, 700 samples x 10 classes, one segment at both caps (500 x 2048), the prepare kernel's rows
  waymo      IoU: grid-aligned and free boxes, 700 segments, one segment at both caps (512 x 512); match: the sparse and the dense
             size grid, the dense grid with scores rounded to eighths (equal scores are common), 700 segments, sparse and dense at both caps
  evaluate   text and dict of the three Python evaluators on the bench tools' synthetic workloads at 300 frames / samples"""
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ENTRY_POINTS = ("eval_overlaps", "eval_match_scores", "eval_match", "nusc_eval_prepare", "nusc_eval_match", "waymo_eval_iou", "waymo_eval_match")


class Recorder:
    """Wraps the seven entry points of toda_amd.ops: every returned tensor goes to out_dir under the current case's name."""

    def __init__(self, ops, out_dir):
        self.ops, self.out_dir, self.case, self.calls = ops, out_dir, "none", 0
        for name in ENTRY_POINTS:
            setattr(ops, name, self.wrap(name, getattr(ops, name)))

    def save(self, name, arr):
        np.save(os.path.join(self.out_dir, f"{self.case}.{name}.npy"), np.asarray(arr))

    def wrap(self, name, fn):
        def call(*args, **kw):
            if name == "waymo_eval_match":
                kw["debug"] = True
            out = fn(*args, **kw)
            outs = [t.cpu().numpy() for t in (out if isinstance(out, tuple) else (out,)) if t is not None]
            if name == "eval_match_scores":                  # scores_out is written for the first counts[f] ground truths of frame f only
                gt_off = args[3].cpu().numpy()
                keep = np.arange(len(outs[0])) < np.repeat(gt_off[:-1] + outs[1], np.diff(gt_off))
                outs[0] = outs[0][keep]
            for k, a in enumerate(outs):
                self.save(f"{self.calls:04d}.{name}.{k}", a)
            self.calls += 1
            return out
        return call

    def result(self, text, res):
        def flat(d, prefix=""):                              # nested dicts (nuScenes: per class and threshold) as "a/b/c" keys
            for k, v in d.items():
                if isinstance(v, dict):
                    yield from flat(v, f"{prefix}{k}/")
                elif isinstance(v, (int, float, np.integer, np.floating)):
                    yield f"{prefix}{k}", float(v)
                else:
                    yield f"{prefix}{k}={v!r}", 0.0
        res = dict(flat(res))
        keys = sorted(res)
        self.save("text", np.array([text]))
        self.save("keys", np.array(keys))
        self.save("values", np.array([float(res[k]) for k in keys], np.float64))


def dump(out_dir):
    sys.path.insert(0, ROOT)
    import torch

    from tests import kitti_eval_cases as KC
    from tests import nusc_eval_cases as NC
    from tests import waymo_eval_cases as WC
    from toda_amd import lib, ops
    from toda_amd.pcdet.datasets.kitti.kitti_object_eval_python import eval as kitti_ev
    from toda_amd.pcdet.datasets.nuscenes import nuscenes_eval as nusc_ev
    from toda_amd.pcdet.datasets.waymo import waymo_eval as waymo_ev
    from toda_amd.tools import bench_kitti_eval, bench_nuscenes_eval, bench_waymo_eval

    os.makedirs(out_dir, exist_ok=True)
    print("tree", ROOT, "library", lib.LIB_PATH, flush=True)
    rec = Recorder(ops, out_dir)
    dev = torch.device("cuda")
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)              # noqa: E731
    gt_sizes, pred_sizes = (0, 1, 63, 64, 65, 129), (0, 1, 2, 64, 65, 500)        # the grids of the GPU tests

    # ---- KITTI
    rec.case = "kitti_frames40"
    gts, dts = KC.kitti_frames(3)
    rec.result(*kitti_ev.get_official_eval_result(gts, dts, ["Car", "Pedestrian", "Cyclist"]))
    rec.case = "kitti_wide"
    gts, dts = KC.kitti_frames(28, 3, classes=("Car", "Van"), mean_gt=45, extra_det=260)
    assert max(len(d["name"]) for d in dts) > 256
    for metric in (0, 1, 2):
        ret = kitti_ev.eval_class(gts, dts, [0, 3], [0, 1, 2], metric, kitti_ev.MIN_OVERLAPS[:, :, [0, 3]], compute_aos=(metric == 0))
        rec.save(f"precision{metric}", ret["precision"])

    # ---- nuScenes
    def nusc_match(segments):
        pred, score, p_attr, gt, g_attr, p_off, g_off, cls = NC.pack_segments(segments)
        ops.nusc_eval_match(up(pred), up(score), up(p_attr), up(gt), up(g_attr), p_off, g_off, cls)

    rec.case = "nusc_size_grid"
    rng, segments = np.random.default_rng(11), []
    for ng in gt_sizes:
        for npred in pred_sizes:
            span = 3 if ng * npred < 5000 else 6
            segments.append((NC.CLASSES[len(segments) % 10], NC.grid_boxes(rng, npred, span, True), NC.grid_boxes(rng, ng, span, False)))
    nusc_match(segments)
    rec.case = "nusc_700_samples"
    rng = np.random.default_rng(7)
    nusc_match([(name, NC.grid_boxes(rng, int(rng.integers(0, 5)), 2, True), NC.grid_boxes(rng, int(rng.integers(0, 4)), 2, False))
                for _ in range(700) for name in NC.CLASSES])
    rec.case = "nusc_at_caps"
    rng = np.random.default_rng(12)
    nusc_match([("barrier", NC.grid_boxes(rng, ops.NUSC_MAX_PRED, 12, True), NC.grid_boxes(rng, ops.NUSC_MAX_GT, 12, False)),
                ("car", NC.grid_boxes(rng, 3, 2, True), NC.grid_boxes(rng, 2, 2, False))])
    rec.case = "nusc_prepare"
    rng = np.random.default_rng(2)
    poses = NC.sample_poses()
    G = np.stack([(np.linalg.inv(c) @ np.linalg.inv(r))[:3] for r, c in poses] + [np.eye(4)[:3]])
    ego = np.stack([np.linalg.inv(c)[:3, 3] for r, c in poses] + [np.zeros(3)])
    n = 1500
    rows = np.concatenate([rng.uniform(-60, 60, (n, 2)), rng.uniform(-3, 2, (n, 1)), rng.uniform(0.3, 8, (n, 3)), rng.uniform(-3.2, 3.2, (n, 1)),
                           rng.uniform(-5, 5, (n, 3))], 1)
    rows[::17, 7:9] = np.nan
    ops.nusc_eval_prepare(up(rows), up(rng.integers(-1, 5, n).astype(np.int32)), up(rng.integers(-1, 11, n).astype(np.int32)), up(G), up(ego))

    # ---- Waymo
    def boxes(rng, n, right_angles, spread=24):
        xyz = rng.integers(-spread, spread + 1, (n, 3)) / 8
        h = rng.integers(-2, 3, (n, 1)) * (np.pi / 2) if right_angles else rng.uniform(-np.pi, np.pi, (n, 1))
        return np.concatenate([xyz, rng.integers(1, 41, (n, 3)) / 8, h], 1)

    def waymo_iou(segments):
        off = lambda k: np.concatenate([[0], np.cumsum([len(s[k]) for s in segments])])          # noqa: E731
        ops.waymo_eval_iou(up(np.concatenate([s[0] for s in segments])), up(np.concatenate([s[1] for s in segments])), off(0), off(1))

    def waymo_match(segments):
        iou, score, ph, gh, level, p_off, g_off, types = WC.pack_segments(segments)
        ops.waymo_eval_match(up(iou), up(score), up(ph), up(gh), up(level), p_off, g_off, types)

    def size_grid(gen, seed):
        rng = np.random.default_rng(seed)
        return [gen(rng, n, m, 1 + (i * len(gt_sizes) + j) % 4) for i, n in enumerate(pred_sizes) for j, m in enumerate(gt_sizes)]

    rng = np.random.default_rng(21)
    rec.case = "waymo_iou_right_angles"
    waymo_iou([(boxes(rng, n, True), boxes(rng, m, True)) for n, m in ((0, 3), (4, 0), (1, 1), (7, 5), (33, 9), (64, 5), (3, 65), (300, 129))])
    rec.case = "waymo_iou_any_angle"
    waymo_iou([(boxes(rng, n, False, 10), boxes(rng, m, False, 10)) for n, m in ((9, 7), (20, 11), (64, 3), (5, 40), (17, 17), (257, 66))])
    rec.case = "waymo_iou_700_segments"
    waymo_iou([(boxes(rng, int(rng.integers(0, 13)), False, 8), boxes(rng, int(rng.integers(0, 9)), False, 8)) for _ in range(700)])
    rec.case = "waymo_iou_at_caps"
    waymo_iou([(boxes(rng, ops.WAYMO_MAX_PRED, False, 40), boxes(rng, ops.WAYMO_MAX_GT, False, 40))])
    rec.case = "waymo_match_sparse_grid"
    waymo_match(size_grid(WC.sparse_segment, 1))
    rec.case = "waymo_match_dense_grid"
    dense = size_grid(WC.dense_segment, 2)
    waymo_match(dense)
    rec.case = "waymo_match_dense_grid_scores_in_eighths"
    waymo_match([(t, iou, (np.round(np.asarray(score, np.float64) * 8) / 8).astype(np.float32), ph, gh, level) for t, iou, score, ph, gh, level in dense])
    rec.case = "waymo_match_700_segments"
    rng = np.random.default_rng(3)
    waymo_match([WC.sparse_segment(rng, int(rng.integers(0, 13)), int(rng.integers(0, 9)), 1 + s % 4) for s in range(700)])
    rec.case = "waymo_match_at_caps"
    rng = np.random.default_rng(4)
    waymo_match([WC.sparse_segment(rng, ops.WAYMO_MAX_PRED, ops.WAYMO_MAX_GT, 2), WC.dense_segment(rng, ops.WAYMO_MAX_PRED, ops.WAYMO_MAX_GT, 1)])

    # ---- the three evaluate() calls on the bench tools' workloads
    rec.case = "evaluate_kitti"
    gts, dts = bench_kitti_eval.make({"frames": 300, "mean_gt": 8, "max_fp": 28, "names": ("car", "pedestrian", "bicycle"), "seed": 1})
    rec.result(*kitti_ev.get_official_eval_result(gts, dts, ["Car", "Pedestrian", "Cyclist"]))
    rec.case = "evaluate_nusc"
    with tempfile.TemporaryDirectory() as tmp:
        infos, dets = bench_nuscenes_eval.make(300, 1, tmp, "v1.0-trainval")
        text, res = nusc_ev.evaluate(infos, dets, list(nusc_ev.CLASSES), tmp, "v1.0-trainval", os.path.join(tmp, "out"))
    rec.result(text, res)
    rec.case = "evaluate_waymo"
    dets, gts = bench_waymo_eval.make(300, 1)
    rec.result(*waymo_ev.evaluate(dets, gts, bench_waymo_eval.CLASS_NAMES))
    print(f"{rec.calls} calls recorded, {len(os.listdir(out_dir))} arrays written", flush=True)


def compare(dir_a, dir_b):
    a, b = sorted(os.listdir(dir_a)), sorted(os.listdir(dir_b))
    if a != b:
        print("file lists differ:", sorted(set(a) ^ set(b)))
        return 1
    differ = []
    for f in a:
        x, y = np.load(os.path.join(dir_a, f)), np.load(os.path.join(dir_b, f))
        if x.dtype != y.dtype or x.shape != y.shape or x.tobytes() != y.tobytes():
            differ.append(f)
            print("DIFFERS", f)
    per = {}
    for f in a:
        per[f.split(".")[0]] = per.get(f.split(".")[0], 0) + 1
    for case, n in per.items():
        print(f"  {case:44s} {n:4d} arrays")
    print(f"compared {len(a)} arrays: {len(differ)} differ (dtype, shape and bytes)")
    return 1 if differ else 0


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "dump":
        dump(sys.argv[2])
    elif len(sys.argv) == 4 and sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    else:
        sys.exit(__doc__)
