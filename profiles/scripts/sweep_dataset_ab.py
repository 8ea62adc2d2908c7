"""Do two checkouts yield the same bits from NuScenesDataset, LyftDataset and NuScenesMixUpAdvDataset.frame_points?

  python profiles/scripts/sweep_dataset_ab.py run TREE_A TREE_B     one fresh child process per tree, then the comparison
  python profiles/scripts/sweep_dataset_ab.py compare A.npz B.npz   two dumps of `child`
  python profiles/scripts/sweep_dataset_ab.py bench TREE_A TREE_B   the frame bench of both trees, five alternating processes each

A tree is a checkout's root (toda_amd/ and tests/); a child imports both packages from its tree only.  TODA_HIP_LIB, when set,
names the library both load.  Each child seeds np.random and torch once, builds the mini trees of tests/nuscenes_dataset_cases.py
and tests/lyft_dataset_cases.py in a temporary directory and dumps, every array under a name:
  * per dataset with MAX_SWEEPS 1 and the tree's own (3 / 5), nuScenes with and without SHIFT_COOR, the training and the
    validation split: raw_frame(k) and ds[k] of every sample, the GT database (every field of every record of the infos pickle,
    every point file), generate_prediction_dicts of one frame with and one without detections, np.random's state afterwards;
  * NuScenesMixUpAdvDataset.frame_points of every labelled and pseudo-labelled info, same settings;
  * np.random's and torch's states at the end.
Arrays are compared as bit patterns (a NaN equals the same NaN).  Exit status 1 when anything differs.  Needs a GPU."""
import os
import pickle
import shutil
import subprocess
import sys
import tempfile
from pathlib import Path

import numpy as np

SHIFT = [0.0, 0.0, 1.8]


def put(out, name, value):
    """value under name: tensors and arrays as they are, dicts and sequences of such member by member."""
    import torch
    if torch.is_tensor(value):
        value = value.detach().cpu().numpy()
    if isinstance(value, dict):
        for key, v in value.items():
            put(out, f"{name}/{key}", v)
        return
    if isinstance(value, (list, tuple)) and any(isinstance(v, (dict, list, tuple, np.ndarray)) or torch.is_tensor(v) for v in value):
        for k, v in enumerate(value):
            put(out, f"{name}/{k}", v)
        return
    arr = np.asarray(value)
    assert name not in out, name
    out[name] = np.array(str(value)) if arr.dtype == object else arr


def dump_dataset(out, tag, ds, preds):
    for k in range(len(ds.infos)):
        put(out, f"{tag}/raw_frame{k}", ds.raw_frame(k))
        put(out, f"{tag}/item{k}", ds[k])
    batch = {"frame_id": ["full", "empty"], "metadata": [{"token": "t0"}, {"token": "t1"}]}
    put(out, f"{tag}/prediction_dicts", ds.generate_prediction_dicts(batch, preds(), ds.class_names))
    put(out, f"{tag}/rng_after", np.random.get_state()[1:])


def dump_database(out, tag, ds, max_sweeps):
    root = Path(ds.root_path)
    before = {p for p in root.rglob("*") if p.is_file()}
    ds.create_groundtruth_database(max_sweeps=max_sweeps)
    for path in sorted({p for p in root.rglob("*") if p.is_file()} - before):
        rel = path.relative_to(root).as_posix()
        if path.suffix == ".pkl":
            with open(path, "rb") as f:
                put(out, f"{tag}/db/{rel}", pickle.load(f))
        else:
            put(out, f"{tag}/db/{rel}", np.fromfile(str(path), np.uint8))
    put(out, f"{tag}/db/rng_after", np.random.get_state()[1:])


def child(tree, out_file):
    sys.path.insert(0, os.path.abspath(tree))
    import torch

    from tests import lyft_dataset_cases as LC
    from tests import nuscenes_dataset_cases as NC
    from toda_amd import lib as L
    from toda_amd.pcdet.datasets import LyftDataset, NuScenesDataset, NuScenesMixUpAdvDataset
    print("package", os.path.dirname(L.__file__), "tests", os.path.dirname(NC.__file__), "library", L.LIB_PATH, flush=True)
    np.random.seed(20240)
    torch.manual_seed(20240)
    rng = np.random.default_rng(3)
    boxes, scores = rng.uniform(-20, 20, (5, 7)).astype(np.float32), rng.uniform(0, 1, 5).astype(np.float32)

    def preds():
        return [{"pred_boxes": torch.from_numpy(boxes.copy()).cuda(), "pred_scores": torch.from_numpy(scores).cuda(), "pred_labels": torch.tensor([1, 2, 9, 1, 3]).cuda()},
                {"pred_boxes": torch.zeros((0, 7)), "pred_scores": torch.zeros(0), "pred_labels": torch.zeros(0, dtype=torch.long)}]

    out = {}
    tmp = Path(tempfile.mkdtemp(prefix="sweep_ab_"))
    try:
        settings = [("nuscenes", NuScenesDataset, NC, sweeps, extra, name) for sweeps in (1, NC.TREE_SWEEPS)
                    for name, extra in (("plain", {}), ("shift", {"SHIFT_COOR": SHIFT}))]
        settings += [("lyft", LyftDataset, LC, sweeps, {}, "plain") for sweeps in (1, LC.TREE_SWEEPS)]
        for n, (kind, cls, cases, sweeps, extra, name) in enumerate(settings):
            data_path = tmp / f"{kind}{n}"
            data_path.mkdir()
            cases.write_tree(data_path)
            tag = f"{kind}/sweeps{sweeps}/{name}"
            for training in (True, False):
                ds = cls(cases.dataset_cfg(data_path, MAX_SWEEPS=sweeps, **extra), cases.CLASSES, training=training)
                dump_dataset(out, f"{tag}/{ds.mode}", ds, preds)
            dump_database(out, tag, cls(cases.dataset_cfg(data_path, MAX_SWEEPS=sweeps, **extra), [], training=True), sweeps)
            if kind == "nuscenes":
                root = data_path / NC.VERSION
                with open(root / "nuscenes_infos_10sweeps_val.pkl", "rb") as f:
                    pseudo = [{**info, "gt_boxes": info["gt_boxes"][:, :7], "p_score": np.full(len(info["gt_boxes"]), 0.8, np.float32)} for info in pickle.load(f)]
                with open(data_path / "pseudo.pkl", "wb") as f:
                    pickle.dump(pseudo, f)
                mix = NuScenesMixUpAdvDataset(NC.dataset_cfg(data_path, DATASET="NuScenesMixUpAdvDataset", MAX_SWEEPS=sweeps, **extra), NC.CLASSES,
                                              training=True, pseudo_info_path=str(data_path / "pseudo.pkl"))
                for k, info in enumerate(mix.infos):
                    put(out, f"{tag}/frame_points{k}", mix.frame_points(info))
                put(out, f"{tag}/frame_points/rng_after", np.random.get_state()[1:])
        put(out, "end/numpy_rng", np.random.get_state()[1:])
        put(out, "end/torch_rng", torch.get_rng_state())
        put(out, "end/torch_cuda_rng", torch.cuda.get_rng_state())
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    np.savez(out_file, **{name.replace("/", "|"): arr for name, arr in out.items()})
    print(f"dumped {len(out)} arrays to {out_file}", flush=True)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def compare(file_a, file_b):
    a, b = np.load(file_a), np.load(file_b)
    if sorted(a.files) != sorted(b.files):
        print("array names differ:", sorted(set(a.files) ^ set(b.files))[:20])
        return 1
    differ = [name for name in sorted(a.files) if not same_bits(a[name], b[name])]
    for name in differ:
        print("DIFFERS", name.replace("|", "/"))
    rng = [name for name in a.files if "rng" in name]
    print(f"compared {len(a.files)} arrays ({sum(a[n].nbytes for n in a.files)} bytes), {len(rng)} of them RNG states: {len(differ)} differ (bit patterns); "
          f"RNG states equal: {not any(n in differ for n in rng)}")
    return 1 if differ else 0


def run(tree_a, tree_b):
    tmp = tempfile.mkdtemp(prefix="sweep_ab_dump_")
    try:
        files = []
        for tag, tree in (("a", tree_a), ("b", tree_b)):
            files.append(os.path.join(tmp, tag + ".npz"))
            subprocess.run([sys.executable, os.path.abspath(__file__), "child", tree, files[-1]], check=True, timeout=600)
        return compare(*files)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def frame_tool(tree, dataset):
    """The frame bench of a tree: bench_sweep_frame --dataset, or the tree's bench_<dataset>_frame where that is all it has."""
    if os.path.exists(os.path.join(tree, "toda_amd", "tools", "bench_sweep_frame.py")):
        return ["toda_amd.tools.bench_sweep_frame", "--dataset", dataset]
    return [f"toda_amd.tools.bench_{dataset}_frame"]


def bench(tree_a, tree_b, runs=5):
    """The frame bench of both trees in alternating fresh processes, A B A B ..., per dataset; medians, A's spread (max - min)
    and the verdict per timing: REGRESSION = B's median worse than A's by more than that spread."""
    import json
    worse = 0
    for dataset, op in (("nuscenes", "sweeps_merge"), ("lyft", "sweeps_merge_rect")):
        got = {"A": [], "B": []}
        for _ in range(runs):
            for tag, tree in (("A", tree_a), ("B", tree_b)):
                done = subprocess.run([sys.executable, "-m", *frame_tool(tree, dataset), "--out", ""], cwd=tree, check=True, timeout=180,
                                      capture_output=True, text=True)
                got[tag].append(json.loads(done.stdout.strip().splitlines()[-1]))
        for label, pick in (("device_chain_ms", lambda r: r[op]["device_chain_ms"]),
                            ("kernel us (wrapper)", lambda r: r[op + "_kernel"]["us_with_output_allocation_and_flag_zeroing"]),
                            ("kernel_large us", lambda r: r[op + "_kernel_large"]["us"])):
            a, b = [pick(r) for r in got["A"]], [pick(r) for r in got["B"]]
            spread, delta = max(a) - min(a), float(np.median(b) - np.median(a))
            worse += delta > spread
            print(f"{dataset:9s}{label:22s}A {a} median {np.median(a):.4f} (spread {spread:.4f})  B {b} median {np.median(b):.4f}  "
                  f"B - A {delta:+.4f}  {'REGRESSION' if delta > spread else 'ok'}", flush=True)
        print(f"{dataset:9s}rows kept / differing from numpy: A {got['A'][0]['rows_kept']} / {got['A'][0]['rows_differing_from_numpy']}, "
              f"B {got['B'][0]['rows_kept']} / {got['B'][0]['rows_differing_from_numpy']}", flush=True)
    print(f"6 timings, {worse} where B is slower than A by more than A's own spread")
    return 0


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "bench":
        sys.exit(bench(sys.argv[2], sys.argv[3]))
    elif len(sys.argv) == 4 and sys.argv[1] == "child":
        child(sys.argv[2], sys.argv[3])
    elif len(sys.argv) == 4 and sys.argv[1] in ("run", "compare"):
        sys.exit((run if sys.argv[1] == "run" else compare)(sys.argv[2], sys.argv[3]))
    else:
        sys.exit(__doc__)
