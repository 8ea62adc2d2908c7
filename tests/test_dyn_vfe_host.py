"""Dynamic VFEs (DynPillarVFE / DynMeanVFE) on the host: configurations build, the CPU restatement matches an independent
numpy / fp64 statement of the reference (pcdet/models/backbones_3d/vfe/dynamic_pillar_vfe.py:95-141,
dynamic_mean_vfe.py:47-76), and the parameter names are the reference's."""
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "toda_amd", "tools", "cfgs", "models", "{}.yaml")

# the MODEL / DATA_PROCESSOR sections of the reference's nuScenes cbgs_dyn_pp_centerpoint.yaml, re-homed on the nuScenes-shape
# synthetic dataset (its ten class names; the synthetic boxes carry no velocity, so the vel head is left out)
NUSC_DYN_PP = """
CLASS_NAMES: ['car','truck', 'construction_vehicle', 'bus', 'trailer', 'barrier', 'motorcycle', 'bicycle', 'pedestrian', 'traffic_cone']
DATA_CONFIG:
    _BASE_CONFIG_: cfgs/dataset_configs/synthetic_nuscenes.yaml
    POINT_CLOUD_RANGE: [-51.2, -51.2, -5.0, 51.2, 51.2, 3.0]
    DATA_PROCESSOR:
        - NAME: mask_points_and_boxes_outside_range
          REMOVE_OUTSIDE_BOXES: True
        - NAME: shuffle_points
          SHUFFLE_ENABLED: {'train': True, 'test': True}
        - NAME: transform_points_to_voxels_placeholder
          VOXEL_SIZE: [0.2, 0.2, 8.0]
MODEL:
    NAME: CenterPoint
    VFE: {NAME: DynPillarVFE, WITH_DISTANCE: False, USE_ABSLOTE_XYZ: True, USE_NORM: True, NUM_FILTERS: [64, 64]}
    MAP_TO_BEV: {NAME: PointPillarScatter, NUM_BEV_FEATURES: 64}
    BACKBONE_2D:
        NAME: BaseBEVBackbone
        LAYER_NUMS: [3, 5, 5]
        LAYER_STRIDES: [2, 2, 2]
        NUM_FILTERS: [64, 128, 256]
        UPSAMPLE_STRIDES: [0.5, 1, 2]
        NUM_UPSAMPLE_FILTERS: [128, 128, 128]
    DENSE_HEAD:
        NAME: CenterHead
        CLASS_AGNOSTIC: False
        CLASS_NAMES_EACH_HEAD: [['car'], ['truck', 'construction_vehicle'], ['bus', 'trailer'], ['barrier'], ['motorcycle', 'bicycle'],
                                ['pedestrian', 'traffic_cone']]
        SHARED_CONV_CHANNEL: 64
        USE_BIAS_BEFORE_NORM: True
        NUM_HM_CONV: 2
        SEPARATE_HEAD_CFG:
            HEAD_ORDER: ['center', 'center_z', 'dim', 'rot']
            HEAD_DICT:
                center: {out_channels: 2, num_conv: 2}
                center_z: {out_channels: 1, num_conv: 2}
                dim: {out_channels: 3, num_conv: 2}
                rot: {out_channels: 2, num_conv: 2}
        TARGET_ASSIGNER_CONFIG: {FEATURE_MAP_STRIDE: 4, NUM_MAX_OBJS: 500, GAUSSIAN_OVERLAP: 0.1, MIN_RADIUS: 2}
        LOSS_CONFIG:
            LOSS_WEIGHTS: {cls_weight: 1.0, loc_weight: 0.25, code_weights: [1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0]}
        POST_PROCESSING:
            SCORE_THRESH: 0.1
            POST_CENTER_LIMIT_RANGE: [-61.2, -61.2, -10.0, 61.2, 61.2, 10.0]
            MAX_OBJ_PER_SAMPLE: 500
            NMS_CONFIG: {NMS_TYPE: nms_gpu, NMS_THRESH: 0.2, NMS_PRE_MAXSIZE: 1000, NMS_POST_MAXSIZE: 83}
    POST_PROCESSING:
        RECALL_THRESH_LIST: [0.3, 0.5, 0.7]
        EVAL_METRIC: synthetic
"""

REF_PFN_KEYS = ["pfn_layers.0.linear.weight", "pfn_layers.0.norm.weight", "pfn_layers.0.norm.bias", "pfn_layers.0.norm.running_mean",
                "pfn_layers.0.norm.running_var", "pfn_layers.0.norm.num_batches_tracked", "pfn_layers.1.linear.weight",
                "pfn_layers.1.norm.weight", "pfn_layers.1.norm.bias", "pfn_layers.1.norm.running_mean", "pfn_layers.1.norm.running_var",
                "pfn_layers.1.norm.num_batches_tracked"]


def load_cfg(name=None, text=None, tmp_path=None, n_points=6000):
    from toda_amd.pcdet.config import AttrDict, cfg_from_yaml_file

    cfg = AttrDict()
    if text is not None:
        path = str(tmp_path / "dyn_pp.yaml")
        open(path, "w").write(text)
        cwd = os.getcwd()
        os.chdir(os.path.join(ROOT, "toda_amd", "tools"))      # _BASE_CONFIG_ paths are relative to tools/
        try:
            cfg_from_yaml_file(path, cfg)
        finally:
            os.chdir(cwd)
    else:
        cfg_from_yaml_file(CFG.format(name), cfg)
    cfg.DATA_CONFIG.SYNTHETIC.NUM_POINTS = n_points
    return cfg


def build(cfg):
    from toda_amd.pcdet.datasets import SyntheticLidarDataset
    from toda_amd.pcdet.models import build_network

    ds = SyntheticLidarDataset(cfg.DATA_CONFIG, cfg.CLASS_NAMES)
    torch.manual_seed(0)
    net = build_network(cfg.MODEL, len(cfg.CLASS_NAMES), ds)
    return ds, net


def cpu_batch(ds, idx=(0, 1)):
    batch = ds.collate_batch([ds[i] for i in idx])
    return {k: (torch.from_numpy(v).float() if isinstance(v, np.ndarray) and k in ("points", "gt_boxes") else v) for k, v in batch.items()}


@pytest.mark.parametrize("source", ["centerpoint_dyn_pillar_waymo", "nusc_dyn_pp", "centerpoint_dyn_voxel_waymo"])
def test_dynamic_configs_build_and_run_on_the_cpu(source, tmp_path):
    cfg = load_cfg(text=NUSC_DYN_PP, tmp_path=tmp_path) if source == "nusc_dyn_pp" else load_cfg(source)
    ds, net = build(cfg)
    assert ds.voxel_cfg.get("dynamic") is True and "max_points_per_voxel" not in ds.voxel_cfg
    vfe_name = cfg.MODEL.VFE.NAME
    assert type(net.vfe).__name__ == {"DynPillarVFE": "DynamicPillarVFE", "DynMeanVFE": "DynamicMeanVFE"}[vfe_name]
    if vfe_name == "DynPillarVFE":
        assert list(ds.grid_size) == ([468, 468, 1] if "waymo" in source else [512, 512, 1])
        assert sorted(net.vfe.state_dict()) == sorted(REF_PFN_KEYS)
        batch = cpu_batch(ds)
        net.train()
        out = net.vfe(dict(batch))
        assert out["pillar_features"].shape[1] == 64 and out["voxel_coords"].shape == (out["pillar_features"].shape[0], 4)
        assert torch.isfinite(out["pillar_features"]).all()
        # the whole dense part on the CPU
        out = net.backbone_2d(net.map_to_bev_module(out))
        assert torch.isfinite(out["spatial_features_2d"]).all()


def test_pseudo_label_perturbation_refuses_dynamic_configs():
    from toda_amd.tools.eval_utils.generate_pseudo_labels_perturb import inference_and_generate_pseudo_labes

    class _DS:
        voxel_cfg = {"point_cloud_range": [0] * 6, "voxel_size": [1, 1, 1], "dynamic": True}

    class _DL:
        dataset = _DS()

    with pytest.raises(NotImplementedError, match="dynamic"):
        inference_and_generate_pseudo_labes(None, None, None, _DL(), None, result_dir=None)


# ---------------------------------------------------------------------------------------------- fp64 restatement of the reference
def np_index(pts, pc_range, vs, grid, pillar):
    """mask, merge key, np.unique (sorted keys, inverse, counts), coords (b, z, y, x), integer cells of the kept points."""
    axes = 2 if pillar else 3
    f = np.floor((pts[:, 1:1 + axes] - np.asarray(pc_range[:axes], np.float32)) / np.asarray(vs[:axes], np.float32))   # fp32 as the reference
    with np.errstate(invalid="ignore"):
        mask = ((f >= 0) & (f < np.asarray(grid[:axes]))).all(1)
    cell = f[mask].astype(np.int64)
    b = pts[mask, 0].astype(np.int64)
    if pillar:
        key = b * grid[0] * grid[1] + cell[:, 0] * grid[1] + cell[:, 1]
    else:
        key = b * grid[0] * grid[1] * grid[2] + cell[:, 0] * grid[1] * grid[2] + cell[:, 1] * grid[2] + cell[:, 2]
    unq, inv, cnt = np.unique(key, return_inverse=True, return_counts=True)
    if pillar:
        sxy = grid[0] * grid[1]
        coords = np.stack([unq // sxy, np.zeros_like(unq), unq % grid[1], (unq % sxy) // grid[1]], 1)
    else:
        sxyz, syz = grid[0] * grid[1] * grid[2], grid[1] * grid[2]
        coords = np.stack([unq // sxyz, unq % grid[2], (unq % syz) // grid[2], (unq % sxyz) // syz], 1)
    return mask, inv.reshape(-1), cnt, coords, cell


def np_pillar_forward(pts, mask, inv, cnt, cell, vs, pc_range, weights, bns):
    """dynamic_pillar_vfe.py:110-141 in fp64 (BN in train mode with the batch statistics, eps 1e-3)."""
    p = pts[mask].astype(np.float64)
    m = len(cnt)
    xyz = p[:, 1:4]
    mean = np.zeros((m, 3))
    np.add.at(mean, inv, xyz)
    mean /= cnt[:, None]
    xo, yo, zo = vs[0] / 2 + pc_range[0], vs[1] / 2 + pc_range[1], vs[2] / 2 + pc_range[2]
    f_center = np.stack([xyz[:, 0] - (cell[:, 0] * vs[0] + xo), xyz[:, 1] - (cell[:, 1] * vs[1] + yo), xyz[:, 2] - zo], 1)
    feats = np.concatenate([p[:, 1:], xyz - mean[inv], f_center], 1)
    deco = feats.copy()
    for li, (w, (g, bb)) in enumerate(zip(weights, bns)):
        x = feats @ w.T
        mu, var = x.mean(0), x.var(0)
        x = np.maximum((x - mu) / np.sqrt(var + 1e-3) * g + bb, 0)
        xmax = np.full((m, x.shape[1]), -np.inf)
        np.maximum.at(xmax, inv, x)
        feats = xmax if li == len(weights) - 1 else np.concatenate([x, xmax[inv]], 1)
    return deco, feats


def random_points(rng, n, bs, pc_range, c=5):
    pts = np.zeros((n, 1 + c), np.float32)
    pts[:, 0] = np.sort(rng.integers(0, bs, n))
    lo, hi = np.asarray(pc_range[:3]), np.asarray(pc_range[3:])
    pts[:, 1:4] = rng.uniform(lo - 0.05 * (hi - lo), hi + 0.05 * (hi - lo), (n, 3))
    pts[:, 4:] = rng.uniform(0, 1, (n, c - 3))
    pts[: n // 3, 1:3] = np.round(pts[: n // 3, 1:3] * 2) / 2      # many points on cell borders
    pts[5] = np.nan
    return pts


def _pillar_vfe(pc_range, vs):
    from toda_amd.pcdet.config import AttrDict
    from toda_amd.pcdet.models.backbones_3d.vfe import __all__ as vfes
    from toda_amd.ops import grid_size_xyz

    cfg = AttrDict({"NAME": "DynPillarVFE", "WITH_DISTANCE": False, "USE_ABSLOTE_XYZ": True, "USE_NORM": True, "NUM_FILTERS": [64, 64]})
    grid = grid_size_xyz(pc_range, vs)
    return vfes["DynPillarVFE"](model_cfg=cfg, num_point_features=5, voxel_size=vs, grid_size=grid, point_cloud_range=pc_range), grid


def test_cpu_dyn_pillar_vfe_matches_fp64_restatement():
    from toda_amd.pcdet.models.backbones_3d.vfe.dynamic_pillar_vfe import torch_dyn_index

    pc_range, vs = [-10.24, -10.24, -2.0, 10.24, 10.24, 4.0], [0.32, 0.32, 6.0]
    torch.manual_seed(1)
    vfe, grid = _pillar_vfe(pc_range, vs)
    vfe.train()
    pts = random_points(np.random.default_rng(0), 4000, 2, pc_range)
    mask, inv, cnt, coords, cell = np_index(pts, pc_range, vs, grid, True)
    out = vfe({"points": torch.from_numpy(pts), "batch_size": 2})
    keep, tinv, tcnt, _, _ = torch_dyn_index(torch.from_numpy(pts), pc_range, vs, grid, 2, True)
    assert np.array_equal(keep.numpy(), mask) and np.array_equal(tinv.numpy(), inv) and np.array_equal(tcnt.numpy(), cnt)
    assert np.array_equal(out["voxel_coords"].numpy(), coords)
    weights = [vfe.pfn_layers[i].linear.weight.detach().double().numpy() for i in range(2)]
    bns = [(vfe.pfn_layers[i].norm.weight.detach().double().numpy(), vfe.pfn_layers[i].norm.bias.detach().double().numpy()) for i in range(2)]
    deco, ref = np_pillar_forward(pts, mask, inv, cnt, cell, vs, pc_range, weights, bns)
    got_deco = vfe.decorate_torch(torch.from_numpy(pts), keep, tinv, _cell(pts, keep, pc_range, vs), len(cnt)).double().numpy()
    assert np.abs(got_deco - deco).max() < 1e-5 * max(1.0, np.abs(deco).max())
    assert np.abs(out["pillar_features"].detach().double().numpy() - ref).max() < 1e-4


def _cell(pts, keep, pc_range, vs):
    t = torch.from_numpy(pts)[keep]
    return torch.floor((t[:, 1:3] - torch.tensor(pc_range[:2], dtype=torch.float32)) / torch.tensor(vs[:2], dtype=torch.float32)).long()


def test_cpu_dyn_mean_vfe_matches_fp64_restatement():
    from toda_amd.pcdet.config import AttrDict
    from toda_amd.pcdet.models.backbones_3d.vfe import __all__ as vfes
    from toda_amd.ops import grid_size_xyz

    pc_range, vs = [-4.0, -4.0, -2.0, 4.0, 4.0, 4.0], [0.1, 0.1, 0.15]
    grid = grid_size_xyz(pc_range, vs)
    vfe = vfes["DynMeanVFE"](model_cfg=AttrDict({"NAME": "DynMeanVFE"}), num_point_features=5, voxel_size=vs, grid_size=grid,
                             point_cloud_range=pc_range)
    pts = random_points(np.random.default_rng(2), 20000, 3, pc_range)
    pts[100:3000, 1:4] = [0.01, 0.02, 0.03]          # a hot cell
    mask, inv, cnt, coords, _ = np_index(pts, pc_range, vs, grid, False)
    out = vfe({"points": torch.from_numpy(pts), "batch_size": 3})
    p = pts[mask, 1:].astype(np.float64)
    mean = np.zeros((len(cnt), p.shape[1]))
    np.add.at(mean, inv, p)
    mean /= cnt[:, None]
    assert np.array_equal(out["voxel_coords"].numpy(), coords)
    assert np.abs(out["voxel_features"].double().numpy() - mean).max() < 1e-6 * max(1.0, np.abs(mean).max())
    assert sorted(vfe.state_dict()) == []


def test_dynamic_geometry_skips_hard_voxelisation():
    from toda_amd.pcdet.models import is_dynamic, voxelize_on_gpu

    cfg = {"point_cloud_range": [0, 0, 0, 1, 1, 1], "voxel_size": [1, 1, 1], "dynamic": True}
    batch = {"points": torch.zeros((4, 6)), "batch_size": 1}
    assert is_dynamic(cfg) and voxelize_on_gpu(batch, cfg) is batch and "voxels" not in batch
    assert not is_dynamic({"max_points_per_voxel": 5})
