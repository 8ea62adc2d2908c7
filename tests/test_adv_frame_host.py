"""NuScenesMixUpAdvDataset and the adversarial-edit entry points without a GPU: the registry, the numpy edit against the
literal restatement of the reference loop (tests/adv_frame_cases.py), the sampling policy, the subset keys and the argument
checks of toda_adv_edit."""
import ctypes
import pickle

import numpy as np
import pytest

from tests import adv_frame_cases as A
from tests import nuscenes_dataset_cases as C
from toda_amd import lib as L


def _cfg(data_path, **extra):
    processor = [{"NAME": "mask_points_and_boxes_outside_range", "REMOVE_OUTSIDE_BOXES": True},
                 {"NAME": "shuffle_points", "SHUFFLE_ENABLED": {"train": True, "test": False}},
                 {"NAME": "transform_points_to_voxels", "VOXEL_SIZE": [0.5, 0.5, 0.5], "MAX_POINTS_PER_VOXEL": 10,
                  "MAX_NUMBER_OF_VOXELS": {"train": 60000, "test": 60000}}]
    return C.dataset_cfg(data_path, DATASET="NuScenesMixUpAdvDataset", MAX_SWEEPS=1, POINT_CLOUD_RANGE=[-10.0, -10.0, -3.0, 70.0, 10.0, 3.0],
                         DATA_PROCESSOR=processor, **extra)


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    """The mini tree with three labelled frames; frames 1 and 2 again as pseudo-labelled infos with scores on both sides of 0.3."""
    path = tmp_path_factory.mktemp("advmix")
    root = C.write_tree(path)
    with open(root / "nuscenes_infos_10sweeps_train.pkl", "rb") as f:
        infos = pickle.load(f)
    pseudo = []
    for info in infos[1:]:
        info = dict(info)
        info["gt_boxes"] = info["gt_boxes"][:, :7].copy()
        info["p_score"] = np.linspace(0.05, 0.9, len(info["gt_boxes"])).astype(np.float32)
        info["p_voxel_coords"], info["p_voxel_perturb"] = np.zeros((0, 3), np.int32), np.zeros((0, 3), np.float32)
        pseudo.append(info)
    with open(path / "pseudo.pkl", "wb") as f:
        pickle.dump(pseudo, f)
    return path


def _dataset(tree, **extra):
    from toda_amd.pcdet.datasets import NuScenesMixUpAdvDataset
    return NuScenesMixUpAdvDataset(_cfg(tree, **extra), C.CLASSES, training=True, pseudo_info_path=str(tree / "pseudo.pkl"))


def test_the_dataset_is_registered_and_marked_as_a_pair_dataset():
    from toda_amd.pcdet import datasets
    cls = datasets.__all__["NuScenesMixUpAdvDataset"]
    assert cls.__name__ == "NuScenesMixUpAdvDataset" and issubclass(cls, datasets.NuScenesDataset)
    assert cls.is_pair_dataset and datasets.SyntheticPairDataset.is_pair_dataset and datasets.SyntheticMixupPairDataset.is_pair_dataset
    assert not getattr(datasets.NuScenesDataset, "is_pair_dataset", False)


HOST_CASES = [(name, lambda name=name: A.objects(A.OBJECT_CASES[name], seed=3 + i)) for i, name in enumerate(A.OBJECT_CASES)]
HOST_CASES += [("lookup", A.lookup_case), ("lookup_absent", lambda: A.lookup_case(absent=True)), ("lookup_no_keys", lambda: A.lookup_case(with_keys=False)),
               ("general_257_2", lambda: A.general(257, 2, 5)), ("general_4099_2", lambda: A.general(4099, 2, 6)), ("boxes_65", lambda: A.many_boxes(65, 7))]


@pytest.mark.parametrize("name,build", HOST_CASES, ids=[c[0] for c in HOST_CASES])
def test_the_numpy_edit_equals_the_literal_loop(tree, name, build):
    ds = _dataset(tree)
    assert [int(g) for g in ds.grid_size] == list(A.GRID)
    case = build()
    want, _, n_kept = A.expected(case)
    got = ds.adversarial_points_host(case["points"].copy(), A.pseudo_info(case), {"op": case["op"], "frac": case["frac"], "seed": case["seed"]})
    assert got.dtype == np.float32 and got.shape == want.shape
    assert got.tobytes() == want.tobytes()
    if name == "lookup":
        assert n_kept == len(case["points"]) and (got[:, :3] != case["points"][:, :3]).any(1).sum() >= 20


def test_boxes_at_or_below_the_threshold_take_no_part_in_the_edit(tree):
    ds = _dataset(tree)
    case = A.objects(A.OBJECT_CASES["one_box_per_op"], seed=9)
    scores = np.array([0.9, 0.3, 0.31, 0.1], np.float32)              # > 0.3 acts: boxes 0 and 2
    draws = {"op": case["op"][[0, 2]], "frac": case["frac"][[0, 2]], "seed": case["seed"][[0, 2]]}
    got = ds.adversarial_points_host(case["points"].copy(), A.pseudo_info(case, scores), draws)
    table = case["table"][[0, 2]]
    rows, _, n_kept, tags = A.literal_edit(case["points"], table, case["keys"], case["grads"])
    assert got.tobytes() == A.in_row_box_order(rows, n_kept, tags).tobytes()


def test_draws_are_three_numbers_per_box_in_box_order(tree):
    ds = _dataset(tree)
    np.random.seed(4)
    draws = ds.draw_edits(3)
    np.random.seed(4)
    for j in range(3):
        assert draws["op"][j] == np.random.randint(3) and draws["frac"][j] == np.random.random()
        assert draws["seed"][j] == np.random.randint(0, 2 ** 32, dtype=np.uint32)
    assert draws["seed"].dtype == np.uint32 and ((draws["frac"] >= 0) & (draws["frac"] < 1)).all()


# ---- sampling policy
def test_repeat_sets_the_length_and_the_infos_are_labelled_then_pseudo(tree):
    ds = _dataset(tree)
    assert len(ds.gt_infos) == 3 and len(ds.ps_infos) == 2 and len(ds.infos) == 5 and len(ds) == 5 and ds.on_device
    assert len(_dataset(tree, REPEAT=7)) == 21
    assert all("p_score" in i for i in ds.infos[3:]) and not any("p_score" in i for i in ds.infos[:3])


@pytest.mark.parametrize("mixup_type,first,second", [("only_gt", "gt", "gt"), ("ps_gt", "ps", "gt"), ("gt_gt+ps", "gt", "any"), ("gt+ps_gt+ps", "any", "any")])
def test_mixup_types_draw_from_the_right_subsets(tree, mixup_type, first, second):
    ds = _dataset(tree, MIXUP_PROB=1.0, MIXUP_TYPE=mixup_type)
    allowed = {"gt": {0, 1, 2}, "ps": {3, 4}, "any": {0, 1, 2, 3, 4}}
    np.random.seed(12)
    seen1, seen2 = set(), set()
    for index in range(200):
        kind, k1, k2 = ds.draw_item(index)
        assert kind == "mixup"
        seen1.add(k1)
        seen2.add(k2)
    assert seen1 == allowed[first] and seen2 == allowed[second]


def test_same_frame_items_follow_mixup_prob_and_gt_prob(tree):
    ds = _dataset(tree, MIXUP_PROB=0.0, GT_PROB=0.5)
    np.random.seed(2)
    picks = [ds.draw_item(index) for index in range(100)]
    assert all(p[0] == "same" for p in picks)
    assert {p[1] for p in picks} == {0, 1, 2, 3, 4}
    for index, p in enumerate(picks):
        assert p[1] == (index % 3 if p[1] < 3 else 3 + index % 2)
    np.random.seed(2)
    assert all(_dataset(tree, MIXUP_PROB=0.0, GT_PROB=1.0).draw_item(i) == ("same", i % 3) for i in range(20))
    assert all(_dataset(tree, MIXUP_TYPE="no_mixup").draw_item(i) == ("same", i % 3) for i in range(20))


def test_mixup_prob_is_the_share_of_mixup_items(tree):
    ds = _dataset(tree, MIXUP_PROB=0.6)
    np.random.seed(8)
    share = np.mean([ds.draw_item(i)[0] == "mixup" for i in range(2000)])
    assert abs(share - 0.6) < 4 * np.sqrt(0.6 * 0.4 / 2000)             # four standard deviations of the binomial share


def test_pseudo_frame_drops_boxes_below_the_threshold(tree):
    ds = _dataset(tree)
    info = dict(ds.ps_infos[0])
    n = len(info["gt_boxes"])
    scores = info["p_score"]
    out = ds.pseudo_frame(dict(info))
    assert len(out["gt_boxes"]) == len(out["gt_names"]) == len(out["p_score"]) == int((scores >= 0.3).sum()) < n
    assert (out["p_score"] >= 0.3).all()
    assert len(ds.pseudo_frame(dict(info), thres=0.0)["gt_boxes"]) == n
    labelled = dict(ds.gt_infos[0])
    assert ds.pseudo_frame(labelled) is labelled and len(labelled["gt_boxes"]) == 17


def test_a_missing_pseudo_file_raises(tree):
    from toda_amd.pcdet.datasets import NuScenesMixUpAdvDataset
    with pytest.raises(FileNotFoundError):
        NuScenesMixUpAdvDataset(_cfg(tree), C.CLASSES, training=True, pseudo_info_path=str(tree / "nothing.pkl"))
    with pytest.raises(ValueError):
        NuScenesMixUpAdvDataset(_cfg(tree), C.CLASSES, training=True)
    ds = NuScenesMixUpAdvDataset(_cfg(tree, PSEUDO_INFO_PATH=str(tree / "pseudo.pkl")), C.CLASSES, training=True)       # the config key serves too
    assert len(ds.ps_infos) == 2


# ---- the subset keys
def test_fmix32_and_the_subset_keys():
    from toda_amd.pcdet.datasets.nuscenes.nuscenes_mixup_adv_dataset import fmix32, subset_keys, subset_size
    assert int(fmix32(0)[0]) == 0
    assert int(fmix32(1)[0]) == 0x514E28B7                                # murmur3's finaliser of 1
    rows = np.arange(5000)
    keys = subset_keys(0xDEADBEEF, rows)
    assert keys.dtype == np.uint32 and (keys == subset_keys(0xDEADBEEF, rows)).all()
    assert (keys == A.row_keys(0xDEADBEEF, rows).astype(np.uint32)).all()
    assert len(np.unique(keys)) == len(rows)                              # a bijection of the row index: no ties inside a box
    assert (keys != subset_keys(0xDEADBEEE, rows)).any()
    assert [subset_size(f, c) for f, c in [(0.0, 7), (0.5, 7), (A.ALMOST_ONE, 7), (0.99, 1), (0.5, 1)]] == [7, 4, 1, 1, 1]


# ---- the C entry points
def _call(table, n=100, c=5, k=None, ws_bytes=None, null=False, voxel=None, grid=None, p=None):
    """toda_adv_edit with fake device pointers that are never dereferenced when the call is refused (or returns early)."""
    lib = L.load()
    k = len(table) if k is None else k
    th = L.host_f64(np.asarray(table, np.float64).reshape(-1))
    lo, vs, gs = L.host_f32(A.LO), L.host_f32(A.VOXEL), L.host_i32(A.GRID)
    ws_bytes = lib.toda_adv_edit_workspace_bytes(n, k) if ws_bytes is None else ws_bytes
    if voxel is not None:
        vs = L.host_f32(voxel)
    if grid is not None:
        gs = L.host_i32(grid)
    dev = None if null else ctypes.c_void_p(256)
    return lib.toda_adv_edit(dev, n, c, L.hptr(th) if len(table) else None, dev, k, None, None, 0, L.hptr(lo), L.hptr(vs), L.hptr(gs), 1e-3,
                             dev, n * 2, dev, dev, dev, ws_bytes, None)


def test_the_entry_points_refuse_bad_arguments_without_a_device():
    lib = L.load()
    good = A.make_table([A.box((0, 0, 0))] * 2, [0, 2], [0.5, 0.0], [1, 2 ** 32 - 1])
    assert lib.toda_adv_edit_max_boxes() >= 512 and lib.toda_adv_edit_chunk() >= 1
    assert lib.toda_adv_edit_workspace_bytes(100000, 40) >= 100000 * (2 * 4 + 2 * 4) + 40 * 256 * 4
    assert _call(good, null=True) == -1 and b"null" in lib.toda_last_error()
    assert _call(good, c=3) == -1 and b"columns" in lib.toda_last_error()
    assert _call(good, n=-1) == -1
    assert _call(good, k=lib.toda_adv_edit_max_boxes() + 1) == -1 and b"boxes" in lib.toda_last_error()
    bad = good.copy()
    bad[1, 7] = 4
    assert _call(bad) == -1 and b"op" in lib.toda_last_error()
    bad = good.copy()
    bad[0, 8] = 1.0
    assert _call(bad) == -1 and b"frac" in lib.toda_last_error()
    bad[0, 8] = -0.1
    assert _call(bad) == -1 and b"frac" in lib.toda_last_error()
    bad[0, 8] = np.nan
    assert _call(bad) == -1 and b"frac" in lib.toda_last_error()
    bad = good.copy()
    bad[0, 9] = 2.0 ** 32
    assert _call(bad) == -1 and b"seed" in lib.toda_last_error()
    assert _call(good, voxel=[0.5, 0.0, 0.5]) == -1 and b"voxel" in lib.toda_last_error()
    assert _call(good, grid=[160, 40, 0]) == -1 and b"grid" in lib.toda_last_error()
    need = lib.toda_adv_edit_workspace_bytes(100, 2)
    assert _call(good, ws_bytes=need - 1) != 0 and b"workspace" in lib.toda_last_error()


def test_the_entry_point_succeeds_without_a_launch_at_n_0_and_k_0():
    good = A.make_table([A.box((0, 0, 0))], [1], [0.5], [7])
    assert _call(good, n=0, null=True) == 0
    assert _call(np.zeros((0, 10)), k=0, null=True) == 0
