#!/usr/bin/env python
"""The labelled-subset files of TODA's target domains: the few per cent of the target's training frames whose annotations
stage 1 and stage 2 may read.  The reference's YAMLs name such files (top_1_percent_frames_kitti_infos_train.pkl,
top_1_percent_frames_nuscenes_infos_10sweeps_train.pkl, ImageSets/train_0.01_1.txt) but it ships no tool that writes them and
does not say how its "top" frames were drawn; this tool draws them uniformly at random with a seed, or takes the first ones.
Pure host code.

    python -m toda_amd.tools.make_labelled_subset kitti <dataset yaml> [--data_path DIR] --percent P [--seed S]
                                                        [--select random|first] [--listing FILE]
    python -m toda_amd.tools.make_labelled_subset nuscenes <dataset yaml> [--data_path DIR] [--version V] --percent P [--seed S]
                                                           [--select random|first]

kitti reads INFO_PATH.train of the yaml under the KITTI root and writes there
    ImageSets/<train split>_<P/100>_<S>.txt             lines `<frame id> <index into the infos>`: what KittiMixUpAdvDataset reads
                                                        (--percent 1 --seed 1: train_0.01_1.txt, the name stage 2 looks for)
    top_<P>_percent_frames_kitti_infos_train.pkl        the infos at those indices in ascending order: stage 1's train infos
--listing FILE builds the pickle from an existing split file instead of drawing (for holders of the authors' lists) and raises
when a listed frame id does not sit at its index.  nuscenes writes top_<P>_percent_frames_nuscenes_infos_10sweeps_train.pkl
from the train infos under <nuScenes root>/<VERSION> in the same way.

The draw: k = max(1, round(n * P / 100)); random: sorted(np.random.default_rng(S).choice(n, k, replace=False)); first: range(k).
"""
import argparse
import pickle
from pathlib import Path

import numpy as np

from ..pcdet.config import AttrDict, cfg_from_yaml_file
from ..pcdet.datasets.kitti.kitti_mixup_adv_dataset import read_labelled_split


def draw_indices(n, percent, seed=1, select="random"):
    """Ascending indices of the labelled subset of n frames."""
    if n < 1:
        raise ValueError("no infos to draw from")
    k = min(n, max(1, round(n * percent / 100)))
    if select == "first":
        return list(range(k))
    if select != "random":
        raise ValueError(f"select = {select}: expected random or first")
    return sorted(int(i) for i in np.random.default_rng(seed).choice(n, k, replace=False))


def _load_infos(root, rels):
    infos = []
    for rel in rels:
        with open(root / rel, "rb") as f:
            infos.extend(pickle.load(f))
    return infos


def _dump(path, infos):
    with open(path, "wb") as f:
        pickle.dump(infos, f)
    print(f"{len(infos)} infos -> {path}")
    return path


def make_kitti_subset(dataset_cfg, root, percent, seed=1, select="random", listing=None):
    """Writes the split file (unless `listing` names one) and the infos pickle under root; returns their paths."""
    root = Path(root)
    infos = _load_infos(root, dataset_cfg.INFO_PATH["train"])
    if listing is not None:
        split_file = Path(listing)
        indices = sorted(read_labelled_split(split_file, infos))       # the check KittiMixUpAdvDataset makes on the same file
    else:
        indices = draw_indices(len(infos), percent, seed, select)
        split_file = root / "ImageSets" / f"{dataset_cfg.DATA_SPLIT['train']}_{percent / 100:g}_{seed}.txt"
        split_file.parent.mkdir(parents=True, exist_ok=True)
        split_file.write_text("".join(f"{infos[i]['point_cloud']['lidar_idx']} {i}\n" for i in indices))
        print(f"{len(indices)} of {len(infos)} frames -> {split_file}")
    return split_file, _dump(root / f"top_{percent:g}_percent_frames_kitti_infos_train.pkl", [infos[i] for i in indices])


def make_nuscenes_subset(dataset_cfg, root, percent, seed=1, select="random"):
    """Writes the infos pickle under root (the directory that holds the train infos: <nuScenes root>/<VERSION>)."""
    root = Path(root)
    infos = _load_infos(root, dataset_cfg.INFO_PATH["train"])
    indices = draw_indices(len(infos), percent, seed, select)
    return _dump(root / f"top_{percent:g}_percent_frames_nuscenes_infos_10sweeps_train.pkl", [infos[i] for i in indices])


def main(argv=None):
    ap = argparse.ArgumentParser(description="write the labelled-subset files of a target domain")
    ap.add_argument("dataset", choices=["kitti", "nuscenes"])
    ap.add_argument("cfg_file", help="dataset yaml, e.g. toda_amd/tools/cfgs/dataset_configs/kitti_dataset.yaml")
    ap.add_argument("--data_path", default=None, help="dataset root; default: DATA_PATH of the yaml")
    ap.add_argument("--version", default=None, help="nuscenes: default VERSION of the yaml")
    ap.add_argument("--percent", type=float, required=True)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--select", choices=["random", "first"], default="random")
    ap.add_argument("--listing", default=None, help="kitti: an existing split file to build the pickle from")
    args = ap.parse_args(argv)
    dataset_cfg = cfg_from_yaml_file(args.cfg_file, AttrDict())
    root = Path(args.data_path or dataset_cfg.DATA_PATH)
    if args.dataset == "kitti":
        return make_kitti_subset(dataset_cfg, root, args.percent, args.seed, args.select, args.listing)
    if args.listing is not None:
        ap.error("--listing belongs to kitti")
    return make_nuscenes_subset(dataset_cfg, root / (args.version or dataset_cfg.VERSION), args.percent, args.seed, args.select)


if __name__ == "__main__":
    main()
