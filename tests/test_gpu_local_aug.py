"""Per-object and pyramid augmentations on the MI355X (csrc/points_local.hip through the C ABI): the device road of
augmentor_utils against the reference's outputs (tests/golden/local_aug.npz) under the assertions the numpy road is held to,
membership masks and keep flags exact, and the three kernels at their edges against this project's numpy road."""
import os

import numpy as np
import pytest
import torch

from tests import local_aug_cases as LA
from toda_amd.pcdet.datasets.augmentor import augmentor_utils as U
from toda_amd.pcdet.utils import common_utils

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def unpack(bits, p):
    words = bits.cpu().numpy().view(np.uint32)
    return ((words[:, np.arange(p) // 32] >> (np.arange(p) % 32).astype(np.uint32)) & 1).astype(bool)


# ---- against the reference ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", LA.case_names())
def test_device_road_matches_the_reference(name):
    c = LA.case(name)
    boxes, points, nxt = LA.run(U, c, c["boxes"], dev(c["points"]))
    assert points.is_cuda
    dev_max = LA.check(c, boxes, points.cpu().numpy(), nxt)
    print(f"{name}: max |device road - reference| = {dev_max:.3e}")


@pytest.mark.parametrize("name", [n for n in LA.case_names() if n.startswith("pyr_")])
def test_membership_masks_and_counts_are_the_references(name):
    from toda_amd import ops
    for pts, pyr, mask in LA.membership_calls(name):
        bits, counts = ops.points_in_pyramids(dev(pts), pyr)
        assert np.array_equal(unpack(bits, len(pyr)), mask)
        assert np.array_equal(counts.cpu().numpy(), mask.sum(0))
        assert np.array_equal(U.points_in_pyramids_mask(dev(pts), pyr).cpu().numpy(), mask)


@pytest.mark.parametrize("name", [n for n in LA.case_names() if "_drop_" in n and not n.startswith("pyr_")])
def test_keep_flags_are_the_references_survivors(name):
    from toda_amd import ops
    c = LA.case(name)
    direction = c["fn"].rsplit("_", 1)[1]
    pts = dev(c["points"])
    np.random.seed(c["seed"])
    if c["fn"].startswith("local"):
        steps = U.local_frustum_dropout_steps(c["boxes"], c["args"][0], direction)
    else:
        intensity = np.random.uniform(*c["args"][0])
        lo, hi = ops.points_column_range(pts, U._DROP[direction][1]).cpu().numpy()
        thr = hi - intensity * (hi - lo) if direction in ("top", "left") else lo + intensity * (hi - lo)
        steps = U._table([U._step(None, U._DROP[direction][0], float(thr), world=True)])
    if len(steps) == 0:
        assert len(c["out_points"]) == len(c["points"])
        return
    out, keep = ops.points_box_steps(pts, steps)
    keep = keep.cpu().numpy().astype(bool)
    assert np.array_equal(out.cpu().numpy(), c["points"])                         # a dropout moves nothing
    assert keep.sum() == len(c["out_points"]) and np.array_equal(c["points"][keep], c["out_points"])


# ---- kernel edges, against the numpy road ---------------------------------------------------------------------------------
def cloud(seed, n, c):
    rng = np.random.default_rng(seed)
    p = rng.uniform(0, 1, (n, c)).astype(np.float32)
    p[:, :3] = p[:, :3] * np.float32([20, 20, 2]) + np.float32([0, -10, -2])
    return p


def step_table(seed, s, ops_allowed, size=(5.0, 11.0)):
    """s steps on random boxes big enough that most steps hit many rows; ops drawn from ops_allowed."""
    from toda_amd import ops
    rng = np.random.default_rng(seed)
    t = np.zeros((s, ops.STEP_COLS), np.float64)
    t[:, 0:3] = np.stack([rng.uniform(0, 20, s), rng.uniform(-10, 10, s), rng.uniform(-1.5, -0.5, s)], 1).astype(np.float32)
    t[:, 3:6] = np.stack([rng.uniform(*size, s), rng.uniform(*size, s), rng.uniform(1, 3, s)], 1).astype(np.float32)
    t[:, 6] = rng.uniform(-np.pi, np.pi, s).astype(np.float32)
    names = rng.choice(ops_allowed, s)
    for i, name in enumerate(names):
        t[i, 7] = ops.STEP_OPS[name]
        if name.startswith("t"):
            t[i, 8] = np.float32(rng.uniform(-0.5, 0.5))
        elif name == "scale":
            t[i, 8] = np.float32(rng.uniform(0.9, 1.1))
        elif name == "rot":
            a = torch.tensor([rng.uniform(-0.3, 0.3)]).float()
            t[i, 8], t[i, 9] = float(torch.cos(a)), float(torch.sin(a))
        else:
            t[i, 8] = np.float32(t[i, 2] + rng.uniform(0.6, 1.2) * (1 if "ge" in name else -1)) if "_z_" in name else \
                np.float32(t[i, 1] + rng.uniform(3, 5) * (1 if "ge" in name else -1))
    return t


def numpy_steps(points, steps):
    """The step table on the host with the expressions of the numpy road (get_points_in_box, fp32 in-place updates)."""
    from toda_amd import ops
    code = {v: k for k, v in ops.STEP_OPS.items()}
    points, alive = points.copy(), np.ones(len(points), bool)
    for row in steps:
        box, name = row[:7].astype(np.float32), code[int(row[7]) & 15]
        mask = alive.copy() if int(row[7]) & ops.STEP_WORLD else U.get_points_in_box(points, box)[1] & alive
        if name in ("tx", "ty", "tz"):
            points[mask, "xyz".index(name[1])] += float(row[8])
        elif name == "scale":
            for a in range(3):
                points[mask, a] -= box[a]
            points[mask, :3] *= float(row[8])
            for a in range(3):
                points[mask, a] += box[a]
        elif name == "rot":
            for a in range(3):
                points[mask, a] -= box[a]
            rot = np.array([[row[8], row[9], 0], [-row[9], row[8], 0], [0, 0, 1]], np.float32)
            points[mask, :3] = points[mask, :3] @ rot
            for a in range(3):
                points[mask, a] += box[a]
        else:
            col = 2 if "_z_" in name else 1
            alive &= ~(mask & (points[:, col] >= row[8] if name.endswith("ge") else points[:, col] <= row[8]))
    return points, alive


EXACT_OPS = ["tx", "ty", "tz", "scale", "drop_z_ge", "drop_z_le", "drop_y_ge", "drop_y_le"]


@pytest.mark.parametrize("c", [4, 5])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257, 5000])
def test_box_steps_edges_match_the_numpy_road(n, c):
    from toda_amd import lib as L
    from toda_amd import ops
    chunk = L.load().toda_points_box_steps_chunk()
    pts = cloud(100 + n, n, c)
    for s in (0, 1, chunk - 1, chunk, chunk + 1, 3 * chunk + 7):
        for allowed in (EXACT_OPS[:4], EXACT_OPS):
            steps = step_table(7 * s + len(allowed), s, allowed)
            want, alive = numpy_steps(pts, steps)
            res = ops.points_box_steps(dev(pts), steps)
            drops = bool((steps[:, 7] >= 5).any())
            assert isinstance(res, tuple) == drops
            got = (res[0] if drops else res).cpu().numpy()
            assert np.array_equal(got[alive], want[alive])                 # bit-equal: the same fp32 operations in the same order
            assert np.array_equal(got[:, 3:], pts[:, 3:])
            if drops:
                assert np.array_equal(res[1].cpu().numpy().astype(bool), alive)
            if n > 1 and s in (1, chunk + 1):
                assert n < 60 or not np.array_equal(got, pts) or s == 1   # the tables do hit rows
    if n >= 257:
        assert not np.array_equal(numpy_steps(pts, step_table(9, 3 * chunk + 7, EXACT_OPS[:4]))[0], pts)


@pytest.mark.parametrize("c", [4, 5])
def test_box_steps_rotation_n_dev_and_out(c):
    from toda_amd import ops
    n, rows = 5000, 3217
    pts, steps = cloud(5, n, c), step_table(6, 70, ["rot", "tx", "scale"])
    want, _ = numpy_steps(pts[:rows], steps)
    n_dev = torch.tensor([rows], dtype=torch.int32, device="cuda")
    fresh = ops.points_box_steps(dev(pts), steps, n_dev=n_dev).cpu().numpy()
    assert np.abs(fresh[:rows].astype(np.float64) - want).max() <= LA.TOL and not np.array_equal(fresh[:rows], pts[:rows])
    assert np.array_equal(fresh[rows:], pts[rows:])                        # rows beyond n_dev come back untouched
    table = dev(pts)
    sentinel = torch.full_like(table, -7.0)
    into = ops.points_box_steps(table, steps, n_dev=n_dev, out=sentinel)
    assert into.data_ptr() == sentinel.data_ptr() and np.array_equal(into.cpu().numpy(), fresh)
    in_place = ops.points_box_steps(table, steps, n_dev=n_dev, out=table)
    assert in_place.data_ptr() == table.data_ptr() and np.array_equal(table.cpu().numpy(), fresh)
    drop = step_table(8, 5, ["drop_z_ge"])
    _, keep = ops.points_box_steps(dev(pts), drop, n_dev=n_dev)
    assert int(keep[rows:].sum()) == 0 and 0 < int(keep.sum()) < rows


def test_chain_where_every_point_sits_in_every_box():
    from toda_amd import ops
    pts = cloud(11, 777, 4)
    steps = step_table(12, 130, ["tx", "ty", "scale"], size=(200.0, 200.0))
    steps[:, 5] = 100.0
    steps[:, 8] = np.where(steps[:, 7] == ops.STEP_OPS["scale"], steps[:, 8], np.float32(0.01))
    want, _ = numpy_steps(pts, steps)
    hits = [U.get_points_in_box(want, r[:7].astype(np.float32))[1].all() for r in steps]
    assert all(hits)
    assert np.array_equal(ops.points_box_steps(dev(pts), steps).cpu().numpy(), want)


def test_a_dropped_point_is_not_moved_again():
    from toda_amd import ops
    pts = cloud(13, 1000, 4)
    box = np.array([10, 0, -1, 100, 100, 50, 0.3], np.float64)
    steps = np.zeros((2, ops.STEP_COLS))
    steps[:, :7] = box
    steps[0, 7], steps[0, 8] = ops.STEP_OPS["drop_z_ge"], -1.0
    steps[1, 7], steps[1, 8] = ops.STEP_OPS["tz"], 5.0                      # would lift every row above the threshold
    out, keep = ops.points_box_steps(dev(pts), steps)
    out, keep = out.cpu().numpy(), keep.cpu().numpy().astype(bool)
    assert np.array_equal(keep, pts[:, 2] < -1.0) and 0 < keep.sum() < len(pts)
    assert np.array_equal(out[~keep], pts[~keep])                           # dropped rows took no further part
    assert np.array_equal(out[keep, 2], pts[keep, 2] + np.float32(5.0))
    want, alive = numpy_steps(pts, steps)
    assert np.array_equal(alive, keep) and np.array_equal(want[keep], out[keep])


@pytest.mark.parametrize("col", [0, 2, 4])
@pytest.mark.parametrize("n", [0, 1, 65, 70000])
def test_column_range(n, col):
    from toda_amd import ops
    pts = cloud(20 + n, n, 5)
    got = ops.points_column_range(dev(pts), col).cpu().numpy()
    want = [pts[:, col].min(), pts[:, col].max()] if n else [np.inf, -np.inf]
    assert np.array_equal(got, np.float32(want))
    if n > 1:
        rows = n // 2
        n_dev = torch.tensor([rows], dtype=torch.int32, device="cuda")
        got = ops.points_column_range(dev(pts), col, n_dev).cpu().numpy()
        assert np.array_equal(got, np.float32([pts[:rows, col].min(), pts[:rows, col].max()]))


@pytest.mark.parametrize("c", [4, 5])
@pytest.mark.parametrize("p", [1, 31, 32, 33, 360])
def test_pyramid_membership_edges(p, c):
    from toda_amd import ops
    t = step_table(30, 60, ["tx"], size=(3.0, 9.0))
    pyr = U.get_pyramids(t[:, :7].astype(np.float32)).reshape(-1, 5, 3)[:p]
    for n in (0, 1, 63, 64, 65, 257, 5000):
        pts = cloud(40 + n, n, c)
        pl = U.pyramid_planes(pyr)
        pl = pl / np.linalg.norm(pl[..., :3], axis=-1, keepdims=True)
        dist = np.einsum("nk,pfk->npf", pts[:, :3].astype(np.float64), pl[..., :3]) - pl[None, :, :, 3]
        pts = np.ascontiguousarray(pts[(np.abs(dist) > 1e-6).all((1, 2))])   # fp64 on both sides, the order of operations differs
        want = U.points_in_pyramids_mask(pts, pyr)
        bits, counts = ops.points_in_pyramids(dev(pts), pyr)
        assert bits.shape == (len(pts), (p + 31) // 32) and np.array_equal(unpack(bits, p), want)
        assert np.array_equal(counts.cpu().numpy(), want.sum(0))
        if len(pts) > 100:
            assert p < 31 or want.any()
            rows = len(pts) // 3
            bits, counts = ops.points_in_pyramids(dev(pts), pyr, torch.tensor([rows], dtype=torch.int32, device="cuda"))
            assert np.array_equal(unpack(bits, p)[:rows], want[:rows]) and not unpack(bits, p)[rows:].any()
            assert np.array_equal(counts.cpu().numpy(), want[:rows].sum(0))


# ---- the whole road -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["local_scale_A", "local_rot_A", "local_drop_top_A", "pyr_aug_A", "pyr_swap_A"])
def test_same_seed_same_bits(name):
    from toda_amd import ops
    c = LA.case(name)
    runs = [LA.run(U, c, c["boxes"].copy(), dev(c["points"])) for _ in range(2)]
    assert np.array_equal(runs[0][0], runs[1][0]) and runs[0][2] == runs[1][2]
    assert torch.equal(runs[0][1], runs[1][1])
    pyr = U.get_pyramids(c["boxes"])
    counts = [ops.points_in_pyramids(dev(c["points"]), pyr)[1] for _ in range(2)]
    assert torch.equal(counts[0], counts[1])


def test_data_augmentor_runs_each_name_on_a_device_cloud():
    from tests.test_local_aug_host import NAMES, augment
    c = LA.case("local_tx_A")
    for name in sorted(NAMES):
        host = augment(name, c["points"].copy(), c["boxes"].copy())
        out = augment(name, dev(c["points"]), c["boxes"].copy())
        assert out["points"].is_cuda and np.array_equal(out["gt_boxes"], host["gt_boxes"])
        got = out["points"].cpu().numpy()
        assert got.shape == host["points"].shape and np.abs(got.astype(np.float64) - host["points"]).max() <= LA.TOL


def test_newaugs_config_trains_one_step():
    from toda_amd.pcdet.config import AttrDict, cfg_from_yaml_file
    from toda_amd.pcdet.datasets import SyntheticLidarDataset
    from toda_amd.pcdet.models import build_network, prepare_batch_on_gpu
    cfg = AttrDict()
    cfg_from_yaml_file(os.path.join(ROOT, "toda_amd", "tools", "cfgs", "models", "pointpillar_newaugs_kitti.yaml"), cfg)
    cfg.DATA_CONFIG.SYNTHETIC.NUM_POINTS = 8000
    ds = SyntheticLidarDataset(cfg.DATA_CONFIG, cfg.CLASS_NAMES, training=True)
    torch.manual_seed(0)
    np.random.seed(0)
    net = build_network(cfg.MODEL, len(cfg.CLASS_NAMES), ds).cuda().train()
    batch = ds.collate_batch([ds[0]])
    prepare_batch_on_gpu(batch, net)
    ret, tb, _ = net(batch)
    assert torch.isfinite(ret["loss"]), tb
    ret["loss"].backward()
    assert all(torch.isfinite(p.grad).all() for p in net.parameters() if p.grad is not None)


def test_wrappers_refuse_strided_tables():
    from toda_amd import ops
    wide = dev(cloud(3, 64, 6))
    steps = step_table(4, 3, ["tx"])
    for view in (wide[:, :4], wide[::2]):
        assert not view.is_contiguous()
        with pytest.raises(RuntimeError, match="contiguous"):
            ops.points_box_steps(view, steps)
        with pytest.raises(RuntimeError, match="contiguous"):
            ops.points_column_range(view, 2)
        with pytest.raises(RuntimeError, match="contiguous"):
            ops.points_in_pyramids(view, np.zeros((1, 15)))
    table = dev(cloud(3, 64, 4))
    with pytest.raises(RuntimeError, match="on the GPU"):
        ops.points_box_steps(table, steps, out=torch.empty(64, 4))
    with pytest.raises(RuntimeError, match="match the table"):
        ops.points_box_steps(table, steps, out=wide[:, :4])
