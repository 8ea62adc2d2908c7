"""Yardstick and inputs of the adversarial-frame tests (tests/test_adv_frame_host.py, tests/test_gpu_adv_frame.py,
tests/test_gpu_nuscenes_mixup_adv.py).  numpy only.

The reference's edit (pcdet/datasets/nuscenes/nuscenes_mixup_adv_dataset.py:191-274) cannot run: its helper module
pcdet/utils/perturb_utils.py is not part of its tree, so there is no capture.  `literal_edit` restates its loop instead: the
index list of every box and the perturbation of every point are computed up front on the frame's coordinates, then the boxes
are visited in order with the reference's statements - x_perturb = points[p_idx, :3] - eps * p_perturb, an assignment for
modify, np.concatenate for add, a dictionary of index lists and one final np.delete for remove.  The only change is where the
random subset comes from: not shuffle()[k:] but the specified key rule, T = the c - k rows smallest in (key(i), i), key(i) =
fmix32(seed ^ uint32(i * 0x9E3779B9)), k = min(floor(frac * c), c - 1).  The box test and the voxel lookup are spelled out in
explicit fp32 steps (the specification's roundings), independent of the library's own helpers.

Every appended row is tagged with (row, box), so the appended block can be put into (row, box) order for the comparison."""
import numpy as np

F32 = np.float32
MASK = np.uint64(0xFFFFFFFF)
MODIFY, ADD, REMOVE, NONE = 0, 1, 2, 3

# the voxel grid of the kernel cases: x in [-10, 70), y in [-10, 10), z in [-3, 3), 0.5 m cells
LO = np.array([-10.0, -10.0, -3.0], F32)
VOXEL = np.array([0.5, 0.5, 0.5], F32)
GRID = (160, 40, 12)
EPS = 1e-3


def fmix32(h):
    h = np.asarray(h, np.uint64) & MASK
    h ^= h >> np.uint64(16)
    h = (h * np.uint64(0x85EBCA6B)) & MASK
    h ^= h >> np.uint64(13)
    h = (h * np.uint64(0xC2B2AE35)) & MASK
    h ^= h >> np.uint64(16)
    return h


def row_keys(seed, rows):
    return fmix32(np.uint64(int(seed)) ^ ((np.asarray(rows, np.uint64) * np.uint64(0x9E3779B9)) & MASK))


def in_box(points, box):
    """get_points_in_box (augmentor_utils.py:474-491) in fp32 steps: |z - cz| <= dz / 2, |local x| <= dx / 2 + 0.1, |local y| likewise."""
    b = np.asarray(box, np.float64).astype(F32)
    x, y, z = points[:, 0].astype(F32), points[:, 1].astype(F32), points[:, 2].astype(F32)
    sx, sy, sz = x - b[0], y - b[1], z - b[2]
    angle = np.float64(-b[6])
    cosa, sina = F32(np.cos(angle)), F32(np.sin(angle))
    lx = sx * cosa + sy * (-sina)
    ly = sx * sina + sy * cosa
    with np.errstate(invalid="ignore"):
        return (np.abs(sz) <= b[5] / F32(2)) & (np.abs(lx) <= b[3] / F32(2) + F32(0.1)) & (np.abs(ly) <= b[4] / F32(2) + F32(0.1))


def voxel_keys_of(coords_zyx, grid):
    c = np.asarray(coords_zyx, np.int64).reshape(-1, 3)
    return (c[:, 0] * grid[1] + c[:, 1]) * grid[0] + c[:, 2]


def point_gradients(xyz, keys_sorted, grads_sorted, lo, voxel, grid):
    """g_i: the stored gradient of the row's voxel; zero outside the grid, for an absent key, with no keys, for a NaN row."""
    xyz = xyz.astype(F32)
    out = np.zeros((len(xyz), 3), F32)
    with np.errstate(invalid="ignore"):
        cell = np.floor((xyz - np.asarray(lo, F32)) / np.asarray(voxel, F32))          # fp32 subtraction, fp32 division
        inside = np.ones(len(xyz), bool)
        for a in range(3):
            inside &= (cell[:, a] >= 0) & (cell[:, a] < grid[a])                        # a NaN compares false
    stored = {int(k): p for p, k in reversed(list(enumerate(keys_sorted)))}             # the first position of a key
    for i in np.nonzero(inside)[0]:
        key = (int(cell[i, 2]) * grid[1] + int(cell[i, 1])) * grid[0] + int(cell[i, 0])
        if key in stored:
            out[i] = grads_sorted[stored[key]]
    return out


def literal_edit(points, table, keys_sorted, grads_sorted, lo=LO, voxel=VOXEL, grid=GRID, eps=EPS):
    """The reference loop.  Returns (rows: the original rows that survive, in order, then the appended rows in the order the
    loop appended them; counts [k]; number of surviving original rows; (row, box) tag of every appended row)."""
    points = np.array(points, F32)
    table = np.asarray(table, np.float64).reshape(-1, 10)
    n = len(points)
    perturb = point_gradients(points[:, :3], keys_sorted, grads_sorted, lo, voxel, grid)
    bbox_pts_idx = [np.nonzero(in_box(points, table[j, :7]))[0] for j in range(len(table))]       # once, up front
    counts = np.array([len(p) for p in bbox_pts_idx], np.int32)
    tags, rm_dict = [], {}
    for j, p_idx in enumerate(bbox_pts_idx):
        p_type, frac, seed, c = int(table[j, 7]), float(table[j, 8]), int(table[j, 9]), len(p_idx)
        if c:
            k = min(int(np.floor(frac * c)), c - 1)
            rand_p_idx = np.lexsort((p_idx, row_keys(seed, p_idx)))[:c - k]       # positions in p_idx of the c - k smallest (key, i)
        if p_type in (MODIFY, ADD) and c > 0:
            x_perturb = points[p_idx, :3].copy() - F32(eps) * perturb[p_idx]
            if p_type == MODIFY:
                points[p_idx[rand_p_idx], :3] = x_perturb[rand_p_idx]
            else:
                new_points = np.concatenate((x_perturb[rand_p_idx], points[p_idx[rand_p_idx], 3:].copy()), axis=1)
                points = np.concatenate((points, new_points))
                tags += [(int(i), j) for i in p_idx[rand_p_idx]]
        elif p_type == REMOVE and c > 5:
            rm_dict[j] = p_idx[rand_p_idx]
    n_kept = n
    if len(rm_dict):
        rm_array = np.array([], dtype="int64")
        for r_idx in rm_dict:
            rm_array = np.concatenate((rm_array, rm_dict[r_idx]))
        points = np.delete(points, rm_array, axis=0)
        n_kept = n - len(np.unique(rm_array))
    return points, counts, n_kept, np.array(tags, np.int64).reshape(-1, 2)


def in_row_box_order(rows, n_kept, tags):
    """The result with its appended block sorted into (row, box) order - the order the device writes."""
    order = np.lexsort((tags[:, 1], tags[:, 0])) if len(tags) else np.zeros(0, np.int64)
    return np.concatenate([rows[:n_kept], rows[n_kept:][order]], 0)


def expected(case):
    rows, counts, n_kept, tags = literal_edit(case["points"], case["table"], case["keys"], case["grads"])
    return in_row_box_order(rows, n_kept, tags), counts, n_kept


# ---- inputs
def background(rng, n, c=5, half=11.0):
    """n rows around the origin (x <= 12: clear of the object boxes at x >= 20); some lie outside the voxel grid."""
    xyz = np.stack([rng.uniform(-half, 12.0, n), rng.uniform(-half, half, n), rng.uniform(-3.5, 3.5, n)], 1)
    return np.concatenate([xyz, rng.uniform(0, 1, (n, c - 3))], 1).astype(F32)


def cluster(rng, centre, n, c=5, spread=(0.4, 0.4, 0.4)):
    xyz = np.asarray(centre) + rng.uniform(-1, 1, (n, 3)) * np.asarray(spread)
    return np.concatenate([xyz, rng.uniform(0, 1, (n, c - 3))], 1).astype(F32)


def box(centre, size=(2.0, 2.0, 2.0), rz=0.3):
    return list(centre) + list(size) + [rz]


def voxel_table(rng, points, share=0.7, lo=LO, voxel=VOXEL, grid=GRID, extra=()):
    """(sorted keys, gradients): the voxels of a random share of the rows inside the grid (and `extra` (z, y, x) cells)."""
    xyz = points[:, :3].astype(F32)
    with np.errstate(invalid="ignore"):
        cell = np.floor((xyz - np.asarray(lo, F32)) / np.asarray(voxel, F32))
        inside = ((cell >= 0) & (cell < np.asarray(grid, F32))).all(1)
    cell = cell[inside & (rng.uniform(0, 1, len(points)) < share)].astype(np.int64)
    coords = np.concatenate([cell[:, ::-1], np.asarray(extra, np.int64).reshape(-1, 3)], 0)
    keys = np.unique(voxel_keys_of(coords, grid))
    return keys.astype(np.int64), (rng.standard_normal((len(keys), 3)) * 100).astype(F32)


def make_table(boxes, op, frac, seed):
    t = np.zeros((len(boxes), 10), np.float64)
    t[:, :7] = np.asarray(boxes, np.float64).reshape(-1, 7)
    t[:, 7], t[:, 8], t[:, 9] = op, frac, seed
    return t


def case(points, boxes, op, frac, seed, keys, grads):
    points = np.ascontiguousarray(points, F32)
    return {"points": points, "boxes": np.asarray(boxes, F32).reshape(-1, 7), "op": np.asarray(op, np.int64), "frac": np.asarray(frac, np.float64),
            "seed": np.asarray(seed, np.int64), "table": make_table(boxes, op, frac, seed), "keys": keys, "grads": grads}


def general(n, k, seed, c=5):
    """n background rows, k large overlapping boxes round the origin with random draws: the edge sizes of the row map."""
    rng = np.random.default_rng(seed)
    pts = background(rng, n, c, half=4.0 if n < 300 else 11.0)
    boxes = [box((0, 0, 0), (10, 10, 4), 0.4), box((3, 2, 0), (8, 6, 3), -0.7)][:k]
    keys, grads = voxel_table(rng, pts)
    return case(pts, boxes, rng.integers(0, 3, k), rng.uniform(0, 1, k), rng.integers(0, 2 ** 32, k), keys, grads)


def many_boxes(k, seed, n=600):
    rng = np.random.default_rng(seed)
    pts = background(rng, n)
    boxes = [box((rng.uniform(-9, 10), rng.uniform(-9, 9), rng.uniform(-1, 1)), rng.uniform(3, 6, 3), rng.uniform(-3, 3)) for _ in range(k)]
    keys, grads = voxel_table(rng, pts)
    return case(pts, boxes, rng.integers(0, 4, k), rng.uniform(0, 1, k), rng.integers(0, 2 ** 32, k), keys, grads)


def objects(spec, seed, n_bg=200, c=5):
    """Background rows and one cluster per entry of spec = [(rows in the cluster, [(op, frac), ...] boxes on it)], the clusters 5 m
    apart from x = 20 on; the background comes first, then the clusters."""
    rng = np.random.default_rng(seed)
    parts, boxes, op, frac = [background(rng, n_bg, c)], [], [], []
    for g, (count, edits) in enumerate(spec):
        centre = (20.0 + 5.0 * g, 0.0, 0.0)
        parts.append(cluster(rng, centre, count, c))
        for o, f in edits:
            boxes.append(box(centre))
            op.append(o)
            frac.append(f)
    pts = np.concatenate(parts, 0)
    keys, grads = voxel_table(rng, pts, share=0.8)
    return case(pts, boxes, op, frac, rng.integers(0, 2 ** 32, len(boxes)), keys, grads)


ALMOST_ONE = 1.0 - 2.0 ** -53

OBJECT_CASES = {
    "one_box_per_op": [(30, [(MODIFY, 0.3)]), (30, [(ADD, 0.6)]), (30, [(REMOVE, 0.5)]), (30, [(NONE, 0.5)])],
    "box_with_no_rows": [(0, [(MODIFY, 0.2)]), (0, [(ADD, 0.2)]), (0, [(REMOVE, 0.2)]), (20, [(ADD, 0.1)])],
    "single_row": [(1, [(MODIFY, 0.99)]), (1, [(ADD, 0.99)]), (1, [(REMOVE, 0.0)])],
    "remove_thresholds": [(5, [(REMOVE, 0.0)]), (6, [(REMOVE, 0.0)]), (6, [(REMOVE, 0.9)])],
    "frac_zero": [(40, [(MODIFY, 0.0)]), (40, [(ADD, 0.0)]), (40, [(REMOVE, 0.0)])],
    "frac_almost_one": [(40, [(MODIFY, ALMOST_ONE)]), (40, [(ADD, ALMOST_ONE)]), (40, [(REMOVE, ALMOST_ONE)])],
    "modify_modify": [(25, [(MODIFY, 0.0), (MODIFY, 0.0)]), (25, [(MODIFY, 0.4), (MODIFY, 0.4)])],
    "modify_add": [(25, [(MODIFY, 0.0), (ADD, 0.0)]), (25, [(MODIFY, 0.4), (ADD, 0.4)])],
    "remove_add": [(25, [(REMOVE, 0.0), (ADD, 0.0)]), (25, [(REMOVE, 0.4), (ADD, 0.4)])],
    "add_remove": [(25, [(ADD, 0.0), (REMOVE, 0.0)]), (25, [(ADD, 0.4), (REMOVE, 0.4)])],
    "add_modify_add_remove_modify": [(50, [(ADD, 0.2), (MODIFY, 0.3), (ADD, 0.5), (REMOVE, 0.6), (MODIFY, 0.1)])],
}


def lookup_case(seed=31, with_keys=True, absent=False):
    """One modify box (frac 0: every row moves by its own gradient) over hand-placed rows: outside the grid on each of the six
    sides, in the first and in the last voxel, on a cell border ((x - lo) / voxel an integer), a NaN row."""
    rng = np.random.default_rng(seed)
    hi = LO + VOXEL * np.asarray(GRID, F32)
    mid = (LO + hi) / 2
    rows = [mid.copy() for _ in range(6)]
    for a in range(3):
        rows[2 * a][a] = LO[a] - 0.25
        rows[2 * a + 1][a] = hi[a] + 0.25
    rows += [LO + 0.25, hi - 0.25, LO + VOXEL * np.array([3, 7, 2], F32), np.array([np.nan, 0.0, 0.0]), np.array([1.0, np.nan, 0.0]), mid]
    pts = np.concatenate([np.asarray(rows, np.float64), rng.uniform(0, 1, (len(rows), 2))], 1).astype(F32)
    pts = np.concatenate([pts, background(rng, 40)], 0)
    everything = box(mid, (hi - LO) + 2.0, 0.0)
    keys, grads = voxel_table(rng, pts, share=0.0 if absent else 1.0, extra=[(5, 5, 5)])
    if not with_keys:
        keys, grads = np.zeros(0, np.int64), np.zeros((0, 3), F32)
    return case(pts, [everything], [MODIFY], [0.0], [12345], keys, grads)


def big_box(seed=41):
    """80 000 rows, 70 000 of them in one region under an add (frac 0.5) and a remove (frac 0.25) box: more rows in a box than
    LDS could hold."""
    rng = np.random.default_rng(seed)
    centre = (40.0, 0.0, 0.0)
    pts = np.concatenate([background(rng, 10000), cluster(rng, centre, 70000, spread=(9.0, 9.0, 1.5))], 0)
    pts = pts[rng.permutation(len(pts))]
    region = box(centre, (20.0, 20.0, 4.0), 0.0)
    keys, grads = voxel_table(rng, pts, share=0.5)
    return case(pts, [region, region], [ADD, REMOVE], [0.5, 0.25], rng.integers(0, 2 ** 32, 2), keys, grads)


def pseudo_info(c, scores=None):
    """A case as the fields of a pseudo-label info: boxes, scores, voxel coordinates (z, y, x) of its keys and gradients."""
    gx, gy = GRID[0], GRID[1]
    keys = c["keys"]
    coords = np.stack([keys // (gx * gy), (keys // gx) % gy, keys % gx], 1).astype(np.int32)
    return {"gt_boxes": c["boxes"].copy(), "gt_names": np.array(["car"] * len(c["boxes"])), "p_score": np.ones(len(c["boxes"]), F32) if scores is None else scores,
            "p_voxel_coords": coords, "p_voxel_perturb": c["grads"].copy()}
