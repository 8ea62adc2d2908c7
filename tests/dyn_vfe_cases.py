"""Input builders and plain references for the dynamic voxel index and the segment kernels of toda_amd/csrc/dynvox.hip (with
radix_sort.cuh and scan.cuh under it), shared by test_dyn_vfe_host.py (no GPU) and test_gpu_dyn_vfe_edges.py.  Everything is
seeded and deterministic.

The specification of the index is the plain-torch torch_dyn_index; the builders here put points where it can also be written down
by hand (cell centres) or where fp32 cell arithmetic is sharpest (the lattice of cell boundaries and their fp32 neighbours).
The segment references restate the contracts of dynvox.hip's header comment: one running fp32 sum per (voxel, column) in seg_pts
order and one fp32 division; a maximum that starts from the segment's first row and is replaced only on `>`.

Out of scope: the radix sort's fourth pass (M > 2^24 voxels; no shipped configuration comes within a factor of five of it) and
NaN inputs of the segmented maximum (the contract does not define their order)."""
import numpy as np
import yaml

from toda_amd import ops

WAYMO_PILLAR = ([-74.88, -74.88, -2.0, 74.88, 74.88, 4.0], [0.32, 0.32, 6.0])
WAYMO_VOXEL = ([-75.2, -75.2, -2.0, 75.2, 75.2, 4.0], [0.1, 0.1, 0.15])
LO_ZERO = ([0.0, -8.0, -2.0, 16.0, 8.0, 4.0], [0.16, 0.16, 6.0])
KITTI_HARD = ([0.0, -39.68, -3.0, 69.12, 39.68, 1.0], [0.16, 0.16, 4.0])      # the hard voxeliser's lo = 0 range
SORT_GRID = ([-48.0, -48.0, -2.0, 48.0, 48.0, 4.0], [0.32, 0.32, 6.0])        # 300 x 300 pillars
WORD_GRID = ([-0.8, -1.12, -2.0, 0.8, 1.12, 4.0], [0.32, 0.32, 6.0])          # 5 x 7 pillars: 105 cells with batch 3
DENORMAL_X = [-0.0, -1e-45, -1e-39, 1e-45]

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


def nusc_dyn_pp_geometry():
    """(range, voxel size) of the nusc_dyn_pp configuration, read from its yaml"""
    cfg = yaml.safe_load(NUSC_DYN_PP)["DATA_CONFIG"]
    vs = [p["VOXEL_SIZE"] for p in cfg["DATA_PROCESSOR"] if "VOXEL_SIZE" in p][0]
    return [float(v) for v in cfg["POINT_CLOUD_RANGE"]], [float(v) for v in vs]


LATTICE_GEOMETRIES = {"waymo_pillar": WAYMO_PILLAR, "waymo_voxel": WAYMO_VOXEL, "nusc_dyn_pp": nusc_dyn_pp_geometry(), "lo_zero": LO_ZERO}


class Geom:
    def __init__(self, pc_range, voxel_size, pillar, batch):
        self.pc_range, self.voxel_size = [float(v) for v in pc_range], [float(v) for v in voxel_size]
        self.pillar, self.batch = bool(pillar), int(batch)
        self.grid = [int(v) for v in ops.grid_size_xyz(pc_range, voxel_size)]
        self.axes = 2 if self.pillar else 3

    @property
    def cells(self):
        """cells of one sample in the key space"""
        return self.grid[0] * self.grid[1] * (1 if self.pillar else self.grid[2])

    def key(self, cells):
        """the merge key of rows (b, x, y, z), int64"""
        c = np.asarray(cells, np.int64).reshape(-1, 4)
        k = (c[:, 0] * self.grid[0] + c[:, 1]) * self.grid[1] + c[:, 2]
        return k if self.pillar else k * self.grid[2] + c[:, 3]

    def cells_of(self, keys):
        """rows (b, x, y, z) of merge keys (z = 0 for pillars)"""
        k = np.asarray(keys, np.int64).reshape(-1)
        z = np.zeros_like(k)
        if not self.pillar:
            k, z = k // self.grid[2], k % self.grid[2]
        return np.stack([k // (self.grid[0] * self.grid[1]), (k // self.grid[1]) % self.grid[0], k % self.grid[1], z], 1)

    def centre(self, cells):
        """fp32 xyz at the centre of cells (b, x, y, z): lo + (c + 1/2) * size in float64, rounded once"""
        c = np.asarray(cells, np.int64).reshape(-1, 4)[:, 1:].astype(np.float64)
        if self.pillar:
            c[:, 2] = 0.0
        lo, vs = np.asarray(self.pc_range[:3]), np.asarray(self.voxel_size)
        if self.pillar:      # the pillar key does not test z: half way up the range
            vs = np.array([vs[0], vs[1], self.pc_range[5] - self.pc_range[2]])
        return (lo + (c + 0.5) * vs).astype(np.float32)


# ---------------------------------------------------------------------------------------------- the boundary lattice
def boundaries(lo, size, grid):
    """fp32(fp64(fp32(lo)) + k * fp64(fp32(size))), k = 0 .. grid: the cell boundaries as the fp32 arithmetic of the index sees its range"""
    return (np.float64(np.float32(lo)) + np.arange(grid + 1) * np.float64(np.float32(size))).astype(np.float32)


def lattice_values(lo, size, grid):
    """[3 * (grid + 1)]: every boundary with its fp32 neighbour below and above.  Holds k = 0 minus one ulp (dropped), k = grid and
    k = grid minus one ulp (past the range and in the last cell on paper; in fp32 (hi - lo) / size may round to either side, and
    torch_dyn_index decides)."""
    b = boundaries(lo, size, grid)
    return np.stack([np.nextafter(b, np.float32(-np.inf)), b, np.nextafter(b, np.float32(np.inf))], 1).reshape(-1)


def boundary_lattice(pc_range, voxel_size, pillar, batch, width=6, extra_x=()):
    """[n, width] rows: for each tested axis (x, y; z too for voxels) its lattice_values, the other axes at the centre of a cell that
    moves with the row (so the rows spread over many cells), the batch column cycling over the samples.  extra_x: more x values."""
    g = Geom(pc_range, voxel_size, pillar, batch)
    rows = []
    for ax in range(g.axes):
        vals = lattice_values(pc_range[ax], voxel_size[ax], g.grid[ax])
        if ax == 0 and len(extra_x):
            vals = np.concatenate([vals, np.asarray(extra_x, np.float32)])
        i = np.arange(len(vals))
        cells = np.stack([i % batch, (7 * i + 3) % g.grid[0], (5 * i + 1) % g.grid[1], (3 * i + 2) % g.grid[2]], 1)
        p = np.zeros((len(vals), width), np.float32)
        p[:, 0] = cells[:, 0]
        p[:, 1:4] = Geom(pc_range, voxel_size, False, batch).centre(cells)
        p[:, 1 + ax] = vals
        p[:, 4:] = (i[:, None] % 17 + np.arange(width - 4)[None, :]) / 32.0
        rows.append(p)
    return np.concatenate(rows)


def reciprocal_moves(pc_range, voxel_size, pillar):
    """how many lattice values land in another cell under fp32 floor((p - lo) * (1 / size)) than under the division"""
    g = Geom(pc_range, voxel_size, pillar, 1)
    moved = 0
    for ax in range(g.axes):
        p = lattice_values(pc_range[ax], voxel_size[ax], g.grid[ax])
        lo, vs = np.float32(pc_range[ax]), np.float32(voxel_size[ax])
        moved += int(np.count_nonzero(np.floor((p - lo) / vs) != np.floor((p - lo) * (np.float32(1) / vs))))
    return moved


# ---------------------------------------------------------------------------------------------- points at cell centres
class CentreCase:
    """pts [n, width] and the index written down by hand: keep [n], inv [K], cnt [M], coords [M, 4] (b, z, y, x), keys [M]"""

    def __init__(self, geom, pts, keep, inv, cnt, coords, keys):
        self.geom, self.pts, self.keep, self.inv, self.cnt, self.coords, self.keys = geom, pts, keep, inv, cnt, coords, keys

    @property
    def M(self):
        return len(self.cnt)

    @property
    def K(self):
        return len(self.inv)


def cell_centres(geom, cells, dup, seed, drop_share=0.25, n_drop=None, width=6):
    """Points at the centres of the distinct `cells` (rows (b, x, y, z)), dup[i] copies of cell i, in a seeded random row order,
    with dropped rows interleaved: out of range in x, NaN x, batch column = batch, in turn.  n_drop (or drop_share of all rows when
    n_drop is None) of the rows are dropped ones."""
    cells = np.asarray(cells, np.int64).reshape(-1, 4)
    dup = np.asarray(dup, np.int64).reshape(-1)
    assert len(cells) == len(dup) and (len(dup) == 0 or dup.min() >= 1)
    keys = geom.key(cells)
    order = np.argsort(keys, kind="stable")
    assert len(np.unique(keys)) == len(keys), "cells must be distinct"
    rank = np.empty(len(keys), np.int64)
    rank[order] = np.arange(len(keys))
    k = int(dup.sum())
    if n_drop is None:
        n_drop = int(np.ceil(k * drop_share / (1.0 - drop_share))) if k else 3
    rng = np.random.default_rng(seed)
    n = k + n_drop
    pts = np.zeros((n, width), np.float32)
    pts[:, 4:] = rng.uniform(0, 1, (n, width - 4)).astype(np.float32)
    voxel = np.concatenate([np.repeat(rank, dup), np.full(n_drop, -1, np.int64)])
    src_cell = np.concatenate([np.repeat(np.arange(len(keys)), dup), rng.integers(0, max(len(keys), 1), n_drop)])
    if len(keys):
        pts[:, 0] = cells[src_cell, 0]
        pts[:, 1:4] = geom.centre(cells[src_cell])
    kind = np.arange(n_drop) % 3
    d = np.arange(k, n)
    pts[d[kind == 0], 1] = np.float32(geom.pc_range[3] + geom.voxel_size[0])
    pts[d[kind == 1], 1] = np.nan
    pts[d[kind == 2], 0] = geom.batch
    perm = rng.permutation(n)
    pts, voxel = pts[perm], voxel[perm]
    keep = voxel >= 0
    c = cells[order]
    coords = np.stack([c[:, 0], np.zeros(len(c), np.int64) if geom.pillar else c[:, 3], c[:, 2], c[:, 1]], 1).astype(np.int32)
    return CentreCase(geom, np.ascontiguousarray(pts), keep, voxel[keep], dup[order].astype(np.int32), coords.reshape(-1, 4), keys[order])


def ragged(m, k, seed):
    """m segment lengths >= 1 that sum to k, unevenly: most of the surplus on a few segments"""
    assert k >= m >= 1
    rng = np.random.default_rng(seed)
    p = rng.uniform(0, 1, m) ** 4 + 1e-9
    return 1 + rng.multinomial(k - m, p / p.sum())


def random_cells(geom, m, seed):
    """m distinct cells (b, x, y, z) of the key space, seeded"""
    keys = np.random.default_rng(seed).choice(geom.cells * geom.batch, size=m, replace=False)
    return geom.cells_of(keys)


# ---- the radix sort's pass count (ceil(bits(M - 1) / 8): 1 pass up to M = 256, 2 up to 65536, then 3) and its ballot ranks
SORT_M = [1, 2, 255, 256, 257, 65535, 65536, 65537]
SORT_M_CASES = [(m, False) for m in SORT_M] + [(m, True) for m in SORT_M if m <= 257]      # (M, ragged duplicates)
SORT_K = [1, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 4097]                             # waves, rounds and tiles of the scatter
SORT_K_CASES = [(k, m) for k in SORT_K for m in (3, 300)]                                   # (K, M); M = min(M, K) voxels


def sort_geom():
    return Geom(*SORT_GRID, True, 2)


def sort_m_case(m, rag):
    g = sort_geom()
    dup = ragged(m, 3 * m + 5, seed=m) if rag else np.ones(m, np.int64)
    return cell_centres(g, random_cells(g, m, seed=m + 1), dup, seed=m + 2)


def sort_k_case(k, m):
    g = sort_geom()
    m = min(m, k)
    return cell_centres(g, random_cells(g, m, seed=k + m), ragged(m, k, seed=k), seed=k + 7 * m)


# ---- scan sizes: n rows, about half dropped; n + 1 keep flags in tiles of 2048, the last three make more than 256 partials
SCAN_N = [2047, 2048, 2049, 524287, 524288, 524289]


def scan_case(n):
    g = sort_geom()
    k = n - n // 2
    m = min(k, 4099)
    return cell_centres(g, random_cells(g, m, seed=n), ragged(m, k, seed=n + 1), seed=n + 2, n_drop=n // 2)


# ---- merge keys above 2^31
WIDE_BATCH = 24


def wide_case(pillar):
    """WAYMO_VOXEL with 24 samples (90 480 640 * 24 keys > 2^31): points in samples 0 and 23, in sample 23 past x cell 1110 (keys
    above 2^31) and in the last cell of the key space.  pillar: the same on the WAYMO_PILLAR grid, whose keys stay below 2^31."""
    g = Geom(*(WAYMO_PILLAR if pillar else WAYMO_VOXEL), pillar, WIDE_BATCH)
    rng = np.random.default_rng(24)
    gx, gy, gz = g.grid
    x_hi = 1110 * gx // 1504

    def some(b, x0, n):
        return np.stack([np.full(n, b), rng.integers(x0, gx, n), rng.integers(0, gy, n), rng.integers(0, gz, n)], 1)

    cells = np.concatenate([some(0, 0, 100), some(23, 0, 100), some(23, x_hi, 100), [[0, 0, 0, 0]], [[23, gx - 1, gy - 1, gz - 1]]])
    if pillar:
        cells[:, 3] = 0
    cells = cells[np.unique(g.key(cells), return_index=True)[1]]
    return cell_centres(g, cells, ragged(len(cells), 3 * len(cells), seed=25), seed=26)


# ---- bitmap word edges: 105 cells, not a multiple of 32
WORD_VARIANTS = {"full": list(range(105)), "edges": [31, 32, 33, 63, 64, 104], "first": [0]}


def word_case(name):
    g = Geom(*WORD_GRID, True, 3)
    keys = WORD_VARIANTS[name]
    return cell_centres(g, g.cells_of(keys), ragged(len(keys), 2 * len(keys) + 3, seed=len(keys)), seed=len(keys) + 1)


# ---- the batch column
def batch_column_case(batch=3):
    """rows at cell centres whose batch column is 0, batch - 1, batch, 0.5, batch - 0.5, -0.0, -0.5, NaN and 1e9, each on several
    cells.  The specification is torch_dyn_index: kept when 0 <= v < batch, then truncated."""
    g = Geom(*WORD_GRID, True, batch)
    vals = np.asarray([0, batch - 1, batch, 0.5, batch - 0.5, -0.0, -0.5, np.nan, 1e9], np.float32)
    case = cell_centres(g, g.cells_of(np.arange(0, 35, 2)), np.full(18, 2), seed=5, n_drop=0)
    pts = np.tile(case.pts, (len(vals), 1))
    pts[:, 0] = np.repeat(vals, len(case.pts))
    return g, pts[np.random.default_rng(6).permutation(len(pts))]


WIDTHS = [4, 6, 7]


def width_case(width):
    g = sort_geom()
    return cell_centres(g, random_cells(g, 300, seed=width), ragged(300, 1000, seed=width + 1), seed=width + 2, width=width)


# ---------------------------------------------------------------------------------------------- hand-built CSR tables
SEG_LENS = [1, 63, 64, 65, 2]      # and one segment of 4097 rows per table


def csr_table(lengths, seed):
    """(seg_off [M + 1], seg_pts [K], inv [K]) int32: rows dealt to the voxels in a seeded random order, each segment ascending"""
    lengths = np.asarray(lengths, np.int64)
    inv = np.random.default_rng(seed).permutation(np.repeat(np.arange(len(lengths)), lengths))
    seg_pts = np.argsort(inv, kind="stable")
    seg_off = np.concatenate([[0], np.cumsum(lengths)])
    return seg_off.astype(np.int32), seg_pts.astype(np.int32), inv.astype(np.int32)


def mixed_lengths(m, rot=0):
    """m segment lengths that run through {1, 63, 64, 65, 2} from position `rot`, one of them (number rot % m) 4097 instead"""
    out = [SEG_LENS[(i + rot) % len(SEG_LENS)] for i in range(m)]
    out[rot % m] = 4097
    return out


def grid_tail_ms(c):
    """voxel counts M whose M * c threads end just below, on (where c divides it) and just above a block of 256, and one with every
    segment length and several blocks"""
    return sorted({max(1, 255 // c), -(-256 // c), -(-257 // c), 12})


def lengths_for_rows(k):
    """segment lengths from {1, 2, 63, 64, 65} (and a remainder) that sum to k"""
    out, i = [], 0
    while k > 0:
        out.append(min(k, [1, 2, 63, 64, 65][i % 5]))
        k -= out[-1]
        i += 1
    return out


# ---------------------------------------------------------------------------------------------- references
def _seq_sum(src, seg_off, seg_pts, rowmap, col0, ncol, divide, dt):
    src = np.asarray(src)
    seg_off, seg_pts = np.asarray(seg_off, np.int64), np.asarray(seg_pts, np.int64)
    lens = np.diff(seg_off)
    out = np.zeros((len(lens), ncol), dt)
    for j in range(int(lens.max(initial=0))):      # the j-th row of every segment that has one: the same order per (voxel, column)
        v = np.nonzero(lens > j)[0]
        r = seg_pts[seg_off[v] + j]
        if rowmap is not None:
            r = np.asarray(rowmap, np.int64)[r]
        out[v] = out[v] + src[r, col0:col0 + ncol].astype(dt)
    return seg_mean(out, seg_off) if divide else out


def seg_mean(sums, seg_off):
    """one division by the segment's row count, in the sums' own precision"""
    return sums / np.diff(np.asarray(seg_off, np.int64))[:, None].astype(sums.dtype)


def seq_sum_f32(src, seg_off, seg_pts, rowmap, col0, ncol, divide):
    """dv_seg_sum_kernel's documented order in numpy float32: one running np.float32 sum per (voxel, column) from 0.0f in seg_pts
    order, then one fp32 division by np.float32(count)"""
    return _seq_sum(src, seg_off, seg_pts, rowmap, col0, ncol, divide, np.float32)


def seq_sum_f64(src, seg_off, seg_pts, rowmap, col0, ncol, divide):
    return _seq_sum(src, seg_off, seg_pts, rowmap, col0, ncol, divide, np.float64)


def seq_sum_bound(src, seg_off, seg_pts, rowmap, col0, ncol, divide, ref64, mag=None):
    """recursive summation of L terms in fp32: |got - ref64| <= L * 2^-24 * sum |x_j| (/ L when dividing), plus one rounding
    2^-24 * |ref64| of the result.  Derived, not measured.  mag: the segments' sum |x_j| where the caller has it already."""
    lens = np.diff(np.asarray(seg_off, np.int64)).astype(np.float64)[:, None]
    if mag is None:
        mag = seq_sum_f64(np.abs(np.asarray(src, np.float64)), seg_off, seg_pts, rowmap, col0, ncol, False)
    return lens * 2.0 ** -24 * mag / (lens if divide else 1.0) + 2.0 ** -24 * np.abs(ref64)


def seg_max_ref(x, seg_off, seg_pts):
    """(max [M, C], arg [M, C] int32): starts from the segment's first row (not from -inf) and is replaced only on `>`, so a tie goes
    to the first row in seg_pts order (all-equal, +0 / -0 and all -inf segments included).  NaN inputs are not defined."""
    x = np.asarray(x, np.float32)
    seg_off, seg_pts = np.asarray(seg_off, np.int64), np.asarray(seg_pts, np.int64)
    lens = np.diff(seg_off)
    assert not np.isnan(x).any() and lens.min(initial=1) >= 1
    arg = np.repeat(seg_pts[seg_off[:-1]][:, None], x.shape[1], 1)
    best = x[seg_pts[seg_off[:-1]]].copy()
    for j in range(1, int(lens.max(initial=0))):
        v = np.nonzero(lens > j)[0]
        r = seg_pts[seg_off[v] + j]
        better = x[r] > best[v]
        best[v] = np.where(better, x[r], best[v])
        arg[v] = np.where(better, r[:, None], arg[v])
    return best, arg.astype(np.int32)


def seg_max_bwd_ref(gout, arg, k):
    """gx [k, C]: gout at the argmax rows, 0.0 everywhere else"""
    gx = np.zeros((k, gout.shape[1]), np.float32)
    gx[arg, np.arange(gout.shape[1])[None, :]] = gout
    return gx


def gather_concat_ref(x, xmax, inv):
    return np.concatenate([x, xmax[np.asarray(inv, np.int64)]], 1)


def decorate_ref64(pts, rows, inv, coords, mean, voxel_size, offsets, use_abs_xyz, with_dist):
    """dynamic_pillar_vfe.py:110-129 in float64: [points[:, 1:] or points[:, 4:], xyz - mean[inv], xyz - pillar centre, (|xyz|)]"""
    p = np.asarray(pts, np.float64)[np.asarray(rows, np.int64)]
    inv, coords = np.asarray(inv, np.int64), np.asarray(coords, np.int64)
    xyz = p[:, 1:4]
    cx, cy = coords[inv, 3], coords[inv, 2]
    centre = np.stack([xyz[:, 0] - (cx * voxel_size[0] + offsets[0]), xyz[:, 1] - (cy * voxel_size[1] + offsets[1]),
                       xyz[:, 2] - offsets[2]], 1)
    parts = [p[:, (1 if use_abs_xyz else 4):], xyz - np.asarray(mean, np.float64)[inv], centre]
    if with_dist:
        parts.append(np.sqrt((xyz * xyz).sum(1, keepdims=True)))
    return np.concatenate(parts, 1)


def decorate_cloud(pc_range, voxel_size, width, seed, n=3000, hot=4097, batch=2):
    """[n + hot, width] points anywhere in the range (so most pillars hold one point, some a few) and `hot` points in one pillar"""
    rng = np.random.default_rng(seed)
    lo, hi = np.asarray(pc_range[:3]), np.asarray(pc_range[3:])
    pts = np.zeros((n + hot, width), np.float32)
    pts[:, 0] = rng.integers(0, batch, n + hot)
    pts[:, 1:4] = rng.uniform(lo - 0.02 * (hi - lo), hi + 0.02 * (hi - lo), (n + hot, 3))
    pts[:, 4:] = rng.uniform(0, 1, (n + hot, width - 4))
    cell_lo = lo[:2] + np.asarray(voxel_size[:2]) * 2
    pts[n:, 0] = 1
    pts[n:, 1:3] = cell_lo + rng.uniform(0.05, 0.95, (hot, 2)) * np.asarray(voxel_size[:2])
    return pts[rng.permutation(n + hot)]
