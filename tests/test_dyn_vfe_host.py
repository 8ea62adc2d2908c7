"""Dynamic VFEs (DynPillarVFE / DynMeanVFE) on the host: configurations build, the CPU restatement matches an independent
numpy / fp64 statement of the reference (pcdet/models/backbones_3d/vfe/dynamic_pillar_vfe.py:95-141,
dynamic_mean_vfe.py:47-76), and the parameter names are the reference's.  Then the edge cases of tests/dyn_vfe_cases.py without a
GPU: the hand-written indices against torch_dyn_index, the segment references against their fp64 / plain-loop twins, the boundary
lattice against a reciprocal multiply, and the argument checks of the eight dynvox entry points, which return their error code with a
message before anything is launched or dereferenced."""
import os

import numpy as np
import pytest
import torch

from tests import dyn_vfe_cases as D
from tests.dyn_vfe_cases import NUSC_DYN_PP
from toda_amd import lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "toda_amd", "tools", "cfgs", "models", "{}.yaml")

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


# ---------------------------------------------------------------------------------------------- the edge cases check themselves
def assert_case_is_its_own_index(case):
    """torch_dyn_index on the case's points gives exactly the index the case wrote down by hand"""
    from toda_amd.pcdet.models.backbones_3d.vfe.dynamic_pillar_vfe import torch_dyn_index

    g = case.geom
    keep, inv, cnt, coords, _ = torch_dyn_index(torch.from_numpy(case.pts), g.pc_range, g.voxel_size, g.grid, g.batch, g.pillar)
    assert coords.shape[0] == case.M and inv.shape[0] == case.K
    assert np.array_equal(keep.numpy(), case.keep) and np.array_equal(inv.numpy(), case.inv)
    assert np.array_equal(cnt.numpy(), case.cnt) and np.array_equal(coords.numpy(), case.coords)
    assert int(case.cnt.sum()) == case.K and np.all(np.diff(case.keys) > 0)


@pytest.mark.parametrize("m,rag", D.SORT_M_CASES)
def test_sort_m_cases_are_their_own_index(m, rag):
    case = D.sort_m_case(m, rag)
    assert case.M == m and (case.K > m or not rag or m == 0) and (rag or case.K == m)
    assert 0 < np.count_nonzero(~case.keep) < len(case.pts)
    assert_case_is_its_own_index(case)


@pytest.mark.parametrize("k,m", D.SORT_K_CASES)
def test_sort_k_cases_are_their_own_index(k, m):
    case = D.sort_k_case(k, m)
    assert case.K == k and case.M == min(m, k)
    assert_case_is_its_own_index(case)


@pytest.mark.parametrize("n", D.SCAN_N)
def test_scan_cases_are_their_own_index(n):
    case = D.scan_case(n)
    assert len(case.pts) == n and case.K == n - n // 2
    assert (-(-(n + 1) // 2048) > 256) == (n >= 524288)      # the keep flags' partial sums need a second sweep of 256; 524287: just not
    # dropped rows are interleaved, not a block at one end
    assert not case.keep[: n // 2].all() and case.keep[: n // 2].any() and case.keep[n // 2:].any()
    assert_case_is_its_own_index(case)


@pytest.mark.parametrize("pillar", [False, True])
def test_wide_key_case_is_its_own_index(pillar):
    case = D.wide_case(pillar)
    assert_case_is_its_own_index(case)
    g = case.geom
    assert g.batch == 24 and (g.cells * g.batch > 2 ** 31) == (not pillar)
    assert case.keys[-1] == g.cells * g.batch - 1 and case.keys[0] == 0
    assert (case.coords[:, 0] == 23).sum() >= 100 and (case.coords[:, 0] == 0).sum() >= 100
    if pillar:
        assert case.keys.max() < 2 ** 31
    else:
        wide = case.keys > 2 ** 31
        assert np.all(case.coords[wide, 0] == 23) and (case.coords[wide, 3] >= 1110).sum() >= 90
        assert tuple(case.coords[-1]) == (23, 39, 1503, 1503)


@pytest.mark.parametrize("name", sorted(D.WORD_VARIANTS))
def test_word_edge_cases_are_their_own_index(name):
    case = D.word_case(name)
    assert case.geom.cells * case.geom.batch == 105 and list(case.keys) == D.WORD_VARIANTS[name]
    assert_case_is_its_own_index(case)


@pytest.mark.parametrize("width", D.WIDTHS)
def test_width_cases_are_their_own_index(width):
    case = D.width_case(width)
    assert case.pts.shape[1] == width
    assert_case_is_its_own_index(case)


def test_batch_column_case_keeps_what_the_reference_keeps():
    """The reference reads the sample as points[:, 0] truncated; torch_dyn_index additionally drops rows outside [0, batch), and
    dv_key does the same: 0, batch - 1, 0.5, batch - 0.5 and -0.0 are kept (samples 0, 2, 0, 2, 0); batch, -0.5, NaN and 1e9 are not."""
    from toda_amd.pcdet.models.backbones_3d.vfe.dynamic_pillar_vfe import torch_dyn_index

    g, pts = D.batch_column_case(3)
    keep, _, cnt, coords, _ = torch_dyn_index(torch.from_numpy(pts), g.pc_range, g.voxel_size, g.grid, 3, True)
    v = pts[:, 0]
    with np.errstate(invalid="ignore"):
        want = (v >= 0) & (v < 3)
    assert np.array_equal(keep.numpy(), want) and want.sum() == 5 * 36
    assert sorted(set(coords[:, 0].tolist())) == [0, 2]
    assert int(cnt[coords[:, 0] == 0].sum()) == 3 * 36 and int(cnt[coords[:, 0] == 2].sum()) == 2 * 36


@pytest.mark.parametrize("name", sorted(D.LATTICE_GEOMETRIES))
def test_boundary_lattice_discriminates_a_reciprocal_multiply(name):
    from toda_amd.pcdet.models.backbones_3d.vfe.dynamic_pillar_vfe import torch_dyn_index

    pc_range, vs = D.LATTICE_GEOMETRIES[name]
    for pillar in (True, False):
        assert D.reciprocal_moves(pc_range, vs, pillar) > 0
    g = D.Geom(pc_range, vs, False, 2)
    extra = D.DENORMAL_X if name == "lo_zero" else ()
    pts = D.boundary_lattice(pc_range, vs, False, 2, extra_x=extra)
    assert len(pts) == 3 * sum(n + 1 for n in g.grid) + len(extra)
    # numpy fp32 and CPU torch agree on every lattice point; the first and the last cell of every axis are hit, lo - 1 ulp is dropped
    keep, _, _, _, cell = torch_dyn_index(torch.from_numpy(pts), pc_range, vs, g.grid, 2, False)
    f = np.floor((pts[:, 1:4] - np.asarray(pc_range[:3], np.float32)) / np.asarray(vs, np.float32))
    with np.errstate(invalid="ignore"):
        mask = ((f >= 0) & (f < np.asarray(g.grid))).all(1)
    assert np.array_equal(keep.numpy(), mask) and np.array_equal(cell.numpy(), f[mask].astype(np.int64))
    at = 0
    for ax in range(3):
        n = 3 * (g.grid[ax] + 1)
        # (which of the three values around the upper bound are kept is fp32's business: (hi - lo) / size may round below the grid)
        k, fa = mask[at:at + n], f[at:at + n, ax]
        assert not k[0] and fa[0] == -1 and k[1] and fa[1] == 0 and k[2] and fa[2] == 0, (name, ax)
        assert g.grid[ax] - 1 in fa[k] and fa[n - 1] in (g.grid[ax] - 1, g.grid[ax])
        at += n + (len(extra) if ax == 0 else 0)
    if name == "lo_zero":      # -0.0 is in cell 0; the negative denormals are below the range
        n = 3 * (g.grid[0] + 1)
        assert list(mask[n:n + 4]) == [True, False, False, True] and f[n, 0] == 0 and f[n + 3, 0] == 0


def test_segment_sum_reference_stays_within_its_bound_of_the_fp64_twin():
    rng = np.random.default_rng(11)
    seg_off, seg_pts, _ = D.csr_table(D.mixed_lengths(12), seed=1)
    k = int(seg_off[-1])
    rowmap = rng.permutation(k + 50)[:k]
    src = (rng.standard_normal((k + 50, 7)) * 10 + 3).astype(np.float32)
    for divide in (False, True):
        for rm in (None, rowmap):
            args = (src, seg_off, seg_pts, rm, 2, 4, divide)
            got, ref = D.seq_sum_f32(*args), D.seq_sum_f64(*args)
            assert got.dtype == np.float32 and got.shape == (12, 4)
            assert np.all(np.abs(got.astype(np.float64) - ref) <= D.seq_sum_bound(*args, ref))
            rows = [seg_pts[seg_off[v]:seg_off[v + 1]] for v in range(12)]
            plain = np.stack([src[r if rm is None else rm[r], 2:6].astype(np.float64).sum(0) / (len(r) if divide else 1) for r in rows])
            assert np.abs(ref - plain).max() <= 1e-9 * np.abs(plain).max()
    # the order is the documented one: 2^24 + 1 + 1 in fp32 stays 2^24 from the front, and is 2^24 + 2 from the back
    off, pts = np.array([0, 3], np.int32), np.array([0, 1, 2], np.int32)
    col = np.array([[2.0 ** 24], [1.0], [1.0]], np.float32)
    assert D.seq_sum_f32(col, off, pts, None, 0, 1, False)[0, 0] == 2.0 ** 24
    assert D.seq_sum_f32(col, off, pts, np.array([2, 1, 0]), 0, 1, False)[0, 0] == 2.0 ** 24 + 2


def test_segment_max_reference_matches_a_plain_loop_and_breaks_ties_low():
    rng = np.random.default_rng(12)
    seg_off, seg_pts, inv = D.csr_table(D.mixed_lengths(12, rot=2), seed=2)
    k = int(seg_off[-1])
    x = rng.permutation(k * 3).reshape(k, 3).astype(np.float32)      # no ties
    best, arg = D.seg_max_ref(x, seg_off, seg_pts)
    ref = torch.segment_reduce(torch.from_numpy(x[seg_pts]), "max", lengths=torch.from_numpy(np.diff(seg_off).astype(np.int64)), axis=0)
    assert np.array_equal(best, ref.numpy())
    assert np.array_equal(x[arg, np.arange(3)[None, :]], best) and np.array_equal(inv[arg], np.repeat(np.arange(12)[:, None], 3, 1))
    # ties: the lowest row, also for +0 / -0 and all -inf
    t = np.zeros((k, 3), np.float32)
    t[:, 0] = -np.inf
    t[::2, 1] = -0.0
    t[:, 2] = rng.integers(0, 2, k)
    best, arg = D.seg_max_ref(t, seg_off, seg_pts)
    first = seg_pts[seg_off[:-1]]
    assert np.array_equal(arg[:, 0], first) and np.array_equal(arg[:, 1], first) and np.all(best[:, 0] == -np.inf)
    assert np.array_equal(np.signbit(best[:, 1]), first % 2 == 0)
    for v in range(12):
        r = seg_pts[seg_off[v]:seg_off[v + 1]]
        assert arg[v, 2] == r[np.argmax(t[r, 2])]      # np.argmax: the first maximum


# ---------------------------------------------------------------------------------------------- argument checks
FAKE = 4096        # a non-null "device pointer" for arguments a refused call must not touch


def refused(rc, *words, code=-1):
    msg = L.load().toda_last_error().decode()
    return rc == code and all(w in msg for w in words)


def _geometry(grid=(468, 468, 1)):
    return L.host_f32([-74.88, -74.88, -2.0]), L.host_f32([0.32, 0.32, 6.0]), L.host_i32(grid)


def _count(lib, n=10, width=6, batch=2, rng=True, vs=True, grid=(468, 468, 1), pillar=1, counts=FAKE, ws=FAKE, ws_bytes=1 << 40):
    r, v, g = _geometry(grid or (1, 1, 1))
    return lib.toda_dynvox_count(FAKE, n, width, batch, L.hptr(r) if rng else None, L.hptr(v) if vs else None, L.hptr(g) if grid else None,
                                 pillar, counts, ws, ws_bytes, None)


def _index(lib, n=10, width=6, batch=2, rng=True, vs=True, grid=(468, 468, 1), pillar=1, m=2, k=5, ws=FAKE, ws_bytes=1 << 40):
    r, v, g = _geometry(grid or (1, 1, 1))
    return lib.toda_dynvox_index(FAKE, n, width, batch, L.hptr(r) if rng else None, L.hptr(v) if vs else None, L.hptr(g) if grid else None,
                                 pillar, m, k, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, ws, ws_bytes, None)


@pytest.mark.parametrize("call", [_count, _index])
def test_dynvox_count_and_index_refuse_bad_geometry_sizes_and_workspace(call):
    lib = L.load()
    for missing in ("rng", "vs", "grid"):
        assert refused(call(lib, **{missing: False}), "dynvox", "required")
    for batch in (0, -1):
        assert refused(call(lib, batch=batch), "batch must be >= 1", "got %d" % batch)
    for grid in ((0, 468, 1), (468, -1, 1), (468, 468, 0)):
        assert refused(call(lib, grid=grid), "grid must be positive")
    # 2^40 keys are refused, for voxels; as pillars the same grid has 2^30 and passes on to the next check
    assert refused(call(lib, grid=(1024, 1024, 1024), batch=1024, pillar=0), "key space", "too large")
    assert refused(call(lib, grid=(1024, 1024, 1024), batch=1024, pillar=1, n=-1), "n=-1")
    assert refused(call(lib, n=-1), "n=-1")
    for width in (3, 0):
        assert refused(call(lib, width=width), "width=%d" % width)
    assert refused(call(lib, ws=None), "null pointer")
    need = lib.toda_dynvox_workspace_bytes(10, 2, L.hptr(L.host_i32((468, 468, 1))), 1) - 256
    assert need > 0
    assert refused(call(lib, ws_bytes=need - 1), "workspace of %d bytes" % (need - 1), "need %d" % need, code=-2)
    assert refused(call(lib, ws_bytes=0), "need %d" % need, code=-2)


def test_dynvox_count_refuses_null_counts():
    assert refused(_count(L.load(), counts=None), "null pointer")


def test_dynvox_index_refuses_inconsistent_sizes():
    lib = L.load()
    for n, k, m in ((10, 11, 2), (10, 5, 6), (10, 0, 1), (10, 5, 0), (10, -1, 0), (10, 5, -1)):
        assert refused(_index(lib, n=n, k=k, m=m), "inconsistent sizes", "k=%d" % k, "m=%d" % m)


def test_dynvox_segment_entry_points_refuse_bad_sizes():
    lib = L.load()
    for ld, col0, ncol in ((6, 0, 0), (6, 0, -1), (6, -1, 3), (6, 4, 3), (6, 0, 7), (3, 3, 1)):
        assert refused(lib.toda_dynvox_seg_sum(FAKE, ld, col0, ncol, None, FAKE, FAKE, 5, 0, FAKE, None), "seg_sum", "rows of %d" % ld)
    assert refused(lib.toda_dynvox_seg_sum(FAKE, 6, 0, 3, None, FAKE, FAKE, -1, 0, FAKE, None), "seg_sum")
    vs, off = L.host_f32([0.32, 0.32]), L.host_f32([0.1, 0.2, 0.3])
    for use_abs in (0, 1):
        for with_dist in (0, 1):
            for width in (4, 6, 7):
                f = width - (1 if use_abs else 4) + 6 + with_dist
                for bad in (f - 1, f + 1, 0):
                    rc = lib.toda_dynvox_pillar_decorate(FAKE, width, FAKE, FAKE, FAKE, FAKE, 9, L.hptr(vs), L.hptr(off), use_abs, with_dist, FAKE,
                                                         bad, None)
                    assert refused(rc, "decorate", "row width %d" % bad, "makes %d" % f)
                # the right width and no rows: nothing to do, null data pointers are fine
                assert lib.toda_dynvox_pillar_decorate(None, width, None, None, None, None, 0, L.hptr(vs), L.hptr(off), use_abs, with_dist, None, f,
                                                       None) == 0
    for width in (3, 0):
        assert refused(lib.toda_dynvox_pillar_decorate(FAKE, width, FAKE, FAKE, FAKE, FAKE, 9, L.hptr(vs), L.hptr(off), 1, 0, FAKE, width + 5, None),
                       "decorate", "bad arguments")
    assert refused(lib.toda_dynvox_pillar_decorate(FAKE, 6, FAKE, FAKE, FAKE, FAKE, 9, None, L.hptr(off), 1, 0, FAKE, 11, None), "bad arguments")
    for c in (0, -1):
        assert refused(lib.toda_dynvox_seg_max_fwd(FAKE, c, FAKE, FAKE, 5, FAKE, FAKE, None), "seg_max", "c=%d" % c)
        assert refused(lib.toda_dynvox_gather_concat(FAKE, FAKE, FAKE, 5, c, FAKE, None), "gather_concat", "c=%d" % c)
        assert refused(lib.toda_dynvox_seg_max_bwd(FAKE, FAKE, 5, c, 9, FAKE, None), "seg_max bwd", "c=%d" % c)
    assert refused(lib.toda_dynvox_seg_max_bwd(FAKE, FAKE, 5, 8, 4, FAKE, None), "seg_max bwd", "m=5", "k=4")
    # with sizes in order, null data pointers are refused before a launch
    assert refused(lib.toda_dynvox_seg_sum(None, 6, 0, 3, None, FAKE, FAKE, 5, 0, FAKE, None), "null pointer")
    assert refused(lib.toda_dynvox_seg_max_fwd(FAKE, 8, FAKE, FAKE, 5, FAKE, None, None), "null pointer")
    assert refused(lib.toda_dynvox_seg_max_bwd(FAKE, FAKE, 5, 8, 9, None, None), "null pointer")
    assert refused(lib.toda_dynvox_gather_concat(FAKE, None, FAKE, 5, 8, FAKE, None), "null pointer")
    assert refused(lib.toda_dynvox_pillar_decorate(FAKE, 6, FAKE, FAKE, FAKE, None, 9, L.hptr(vs), L.hptr(off), 1, 0, FAKE, 11, None), "null pointer")


def test_dynvox_segment_entry_points_accept_the_empty_cases_with_null_pointers():
    lib = L.load()
    assert lib.toda_dynvox_seg_sum(None, 6, 1, 3, None, None, None, 0, 1, None, None) == 0
    assert lib.toda_dynvox_seg_max_fwd(None, 8, None, None, 0, None, None, None) == 0
    assert lib.toda_dynvox_seg_max_bwd(None, None, 0, 8, 0, None, None) == 0
    assert lib.toda_dynvox_gather_concat(None, None, None, 0, 8, None, None) == 0


def test_dynvox_workspace_bytes():
    lib = L.load()
    grid = L.host_i32((468, 468, 1))
    assert lib.toda_dynvox_workspace_bytes(-1, 2, L.hptr(grid), 1) == 0
    assert lib.toda_dynvox_workspace_bytes(10, 0, L.hptr(grid), 1) == 0
    assert lib.toda_dynvox_workspace_bytes(10, 2, None, 1) == 0
    sizes = [lib.toda_dynvox_workspace_bytes(n, 2, L.hptr(grid), 1) for n in (0, 1, 255, 256, 257, 2047, 2048, 2049, 65536, 524288, 524289, 1 << 22)]
    assert sizes[0] > 0 and all(b >= a for a, b in zip(sizes, sizes[1:])) and sizes[-1] > sizes[0]
    # every point needs its keep position, its key and two (key, value) pairs
    assert sizes[-1] - sizes[0] >= (1 << 22) * (4 + 8 + 16)
    g = D.wide_case(False).geom
    words = -(-g.cells * g.batch // 32)
    assert g.cells * g.batch > 2 ** 31 and 8 * words > 2 ** 29
    assert lib.toda_dynvox_workspace_bytes(300, g.batch, L.hptr(L.host_i32(g.grid)), 0) >= 8 * words      # no 32-bit wrap
