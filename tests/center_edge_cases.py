"""Case builders and references of the CenterPoint head's kernels (csrc/center_assign.hip, center_loss.hip, rotated_overlap.cuh,
nms.hip), shared by test_center_edges_host.py (no GPU), test_gpu_center_edges.py and golden/capture_center_edges.py.

  assign    the case table and gt builders of tests/golden/center_edges.npz, whose expected outputs are the reference's own
            CenterHead.assign_targets (captured by golden/capture_center_edges.py)
  loss      the case table of the fused centre loss; its reference is torch_losses of test_gpu_center_loss.py in float64
  overlap   a float64 Sutherland-Hodgman clip of two rotated rectangles written from the definition (it shares nothing with the
            kernel or the oracle, which both collect crossings and inside corners and sort them by angle), closed forms, and
            seeded random pairs kept away from the configurations where the reference algorithm's margins decide the result
  nms       lattices of disjoint boxes with planted duplicates and chains; the keep lists follow from the construction
"""
import math

import numpy as np

# ====================================================================================================== target assignment
CLASSES = ["Vehicle", "Pedestrian", "Cyclist"]
STRIDE, VOXEL, OVERLAP = 8, [0.125, 0.125, 0.15], 0.1           # one cell of the map = 1 m x 1 m

ONE_HEAD = [["Vehicle", "Pedestrian", "Cyclist"]]
# name: H x W map, gt rows, code (= gt columns: 7 box + velocity columns + class), NUM_MAX_OBJS, MIN_RADIUS, heads, samples, seed
ASSIGN_CASES = {
    # non-square map; ~225 in-head boxes over a cap of 150: the second chunk of 256 rows lies entirely past the cap; rb[8:10]
    "wide": dict(h=12, w=20, g=300, code=10, max_objs=150, min_radius=2, heads=ONE_HEAD, batch=2, seed=101),
    # the transposed map; rows >= 256 are drawn at a slot that continues the first chunk's count; planted rows (plant_tall)
    "tall": dict(h=20, w=12, g=300, code=8, max_objs=500, min_radius=2, heads=ONE_HEAD, batch=3, seed=102),
    # radius >= 4 on a 3 x 5 map: every window is clipped on all four sides
    "tiny": dict(h=3, w=5, g=40, code=8, max_objs=500, min_radius=4, heads=ONE_HEAD, batch=2, seed=103),
    # a one-cell map, cap 3
    "cell": dict(h=1, w=1, g=7, code=10, max_objs=3, min_radius=2, heads=ONE_HEAD, batch=2, seed=104),
    # per-head compaction, both heads over the cap
    "two_heads": dict(h=12, w=20, g=270, code=10, max_objs=60, min_radius=2, heads=[["Vehicle"], ["Pedestrian", "Cyclist"]],
                      batch=2, seed=105),
    # no gt rows at all
    "empty": dict(h=12, w=20, g=0, code=8, max_objs=10, min_radius=2, heads=ONE_HEAD, batch=2, seed=106),
}
# rows of sample 0 of `tall` that plant_tall overwrites
TALL_DX0, TALL_TWICE, TALL_BLEND, TALL_CELL = 3, (10, 11), (20, 21), (30, 31)
TALL_CLASS0_SAMPLE = 2


def assign_geometry(case):
    """(pc_range, voxel_size, grid_size) of a case: the range starts at 0 and spans W x H metres."""
    c = ASSIGN_CASES[case]
    pc_range = np.array([0, 0, -2, c["w"], c["h"], 4], np.float32)
    return pc_range, list(VOXEL), np.array([c["w"] * STRIDE, c["h"] * STRIDE, 40])


def assign_gt(case):
    """gt [batch, g, code] float32: centres uniform in [-0.1, 1.1] of the extent (some clamp at each border), classes 0..3
    (0: in no head), the last five rows of sample 1 zeroed as padding."""
    c = ASSIGN_CASES[case]
    rng = np.random.default_rng(c["seed"])
    b, g, code = c["batch"], c["g"], c["code"]
    gt = np.zeros((b, g, code), np.float32)
    gt[:, :, 0] = rng.uniform(-0.1, 1.1, (b, g)) * c["w"]
    gt[:, :, 1] = rng.uniform(-0.1, 1.1, (b, g)) * c["h"]
    gt[:, :, 2] = rng.uniform(-1, 2, (b, g))
    gt[:, :, 3:6] = rng.uniform(0.3, 4.0, (b, g, 3))
    gt[:, :, 6] = rng.uniform(-3.14, 3.14, (b, g))
    gt[:, :, 7:code - 1] = rng.standard_normal((b, g, code - 8))
    gt[:, :, code - 1] = rng.integers(0, 4, (b, g))
    if g >= 5:
        gt[1, g - 5:] = 0
    if case == "tall":
        plant_tall(gt)
    return gt


def plant_tall(gt):
    s = gt[0]
    s[TALL_DX0, 3], s[TALL_DX0, 7] = 0.0, 1                    # dx = 0: not drawn, but it keeps its slot
    a, b = TALL_TWICE                                           # one box twice, same class
    s[a, 0:2], s[a, 7] = (5.3, 9.6), 2
    s[b] = s[a]
    a, b = TALL_BLEND                                           # two sizes on one centre, same class: the max-blend
    s[a, 0:2], s[a, 3:5], s[a, 7] = (7.5, 14.25), (3.9, 3.7), 3
    s[b] = s[a]
    s[b, 3:5] = (0.6, 0.5)
    a, b = TALL_CELL                                            # two classes in one cell
    s[a, 0:2], s[a, 7] = (2.2, 3.3), 1
    s[b, 0:2], s[b, 7] = (2.7, 3.8), 2
    gt[TALL_CLASS0_SAMPLE, :, 7] = 0                            # a sample with nothing in any head


def head_gt(gt, case, head):
    """gt with the class column remapped to 1..len(head's names), 0 for a class outside that head."""
    names = ASSIGN_CASES[case]["heads"][head]
    lut = np.zeros(len(CLASSES) + 1, np.float32)
    for i, n in enumerate(CLASSES):
        if n in names:
            lut[i + 1] = names.index(n) + 1
    out = np.array(gt, np.float32, copy=True)
    out[..., -1] = lut[gt[..., -1].astype(np.int64)]
    return out


def head_cfg(case):
    """The TARGET_ASSIGNER_CONFIG / CLASS_NAMES_EACH_HEAD overrides of a case on top of the golden HEAD_CFG."""
    c = ASSIGN_CASES[case]
    return dict(CLASS_NAMES_EACH_HEAD=c["heads"],
                TARGET_ASSIGNER_CONFIG=dict(FEATURE_MAP_STRIDE=STRIDE, NUM_MAX_OBJS=c["max_objs"], GAUSSIAN_OVERLAP=OVERLAP,
                                            MIN_RADIUS=c["min_radius"]))


# ====================================================================================================== fused centre loss
# name: (B, C, H, W, K, branch channels), and what the case is for.  The builder is loss_case below.
LOSS_CASES = {
    "no_positive": (2, 3, 12, 20, 7, (2, 1, 3, 2)),            # no heat-map cell equals 1: num_pos clamps to 1
    "all_masked": (2, 3, 12, 20, 7, (2, 1, 3, 2)),             # mask all zero: num_obj clamps to 1, loc_loss and its gradients are 0
    "k1": (2, 2, 5, 7, 1, (2, 1, 3, 2)),
    "one_cell_300": (2, 1, 6, 9, 300, (2, 1, 3, 2)),           # every slot on one cell, K > 256: the owner search crosses the stride
    "d16": (2, 2, 6, 10, 9, (2, 2, 2, 2, 2, 2, 2, 2)),         # CL_MAX_DIM over CL_MAX_BRANCH
    "n1024": (2, 4, 8, 16, 11, (2, 1, 3, 2)),                  # B*C*H*W = one block of the heat-map pass exactly
    "n2048": (4, 4, 8, 16, 11, (2, 1, 3, 2)),                  # ... and two
    "last_cell": (2, 3, 12, 20, 7, (2, 1, 3, 2)),              # a slot on cell H*W - 1 of a non-square map
    "k8192": (1, 1, 4, 4, 8192, (2, 1, 3, 2)),                 # the largest K the entry point accepts
}
LOSS_K_MAX = 8192
LOSS_BLOCK_ELEMS = 1024                                         # CL_BLOCK * CL_ITEMS of center_loss.hip


def loss_case(name):
    """CPU tensors (hm, heatmap, inds, mask, target, regs) of a LOSS_CASES entry, built like test_gpu_center_loss.py builds its
    geometries: logits on both clamp sides, slots that share a cell, empty slots on cell 0, positives under the live slots."""
    import torch

    b, c, h, w, k, chans = LOSS_CASES[name]
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    hm = torch.randn((b, c, h, w), generator=g) * 3 - 2
    hm[0, 0, 0, :4] = torch.tensor([-20.0, 20.0, -9.3, 9.3])
    heatmap = torch.rand((b, c, h, w), generator=g).pow(6).clamp_(max=0.96875)
    d = sum(chans)
    inds = torch.randint(0, h * w, (b, k), generator=g)
    mask = (torch.rand((b, k), generator=g) < 0.4).long()
    mask[:, :2] = 1
    if k > 1:
        inds[:, 1] = inds[:, 0]
    if name == "one_cell_300":
        inds[:] = torch.tensor([h * w // 2, 3])[:, None]
        mask[:] = 1
    if name == "k8192":
        mask[:] = (torch.rand((b, k), generator=g) < 0.9).long()
    if name == "last_cell":
        inds[:, 0] = h * w - 1
        inds[:, 1] = h * w - 1
        inds[0, 2], mask[0, 2] = h * w - w, 1                  # first cell of the last row
    if name == "all_masked":
        mask[:] = 0
    inds[mask == 0] = 0
    if name != "no_positive":
        for bi in range(b):
            cells = inds[bi][mask[bi] == 1]
            heatmap[bi, torch.randint(0, c, (len(cells),), generator=g), cells // w, cells % w] = 1.0
        if name == "all_masked":
            heatmap[0, 0, 1, 1] = 1.0                          # positives exist, objects do not
    target = torch.randn((b, k, d), generator=g)
    regs = [torch.randn((b, ch, h, w), generator=g) for ch in chans]
    return hm, heatmap, inds, mask, target, regs


# ====================================================================================================== rotated overlap
def corners64(box):
    """The four corners of (x, y, z, dx, dy, dz, heading), counter-clockwise, in float64 from the box's own (float32) numbers."""
    x, y, dx, dy, r = (float(box[i]) for i in (0, 1, 3, 4, 6))
    c, s = math.cos(r), math.sin(r)
    return [(x + lx * c - ly * s, y + lx * s + ly * c) for lx, ly in ((-dx / 2, -dy / 2), (dx / 2, -dy / 2), (dx / 2, dy / 2), (-dx / 2, dy / 2))]


def clip_area(a, b):
    """Area of the intersection of two rotated rectangles: Sutherland-Hodgman, polygon a clipped by the four half-planes of b,
    then the shoelace formula.  A rectangle without area has an empty interior."""
    if not (float(a[3]) > 0 and float(a[4]) > 0 and float(b[3]) > 0 and float(b[4]) > 0):
        return 0.0
    poly, clip = corners64(a), corners64(b)
    for i in range(4):
        (x0, y0), (x1, y1) = clip[i], clip[(i + 1) % 4]
        ex, ey = x1 - x0, y1 - y0
        side = [ex * (py - y0) - ey * (px - x0) for px, py in poly]      # >= 0: left of the edge, i.e. inside
        out = []
        for k in range(len(poly)):
            p, q, sp, sq = poly[k], poly[(k + 1) % len(poly)], side[k], side[(k + 1) % len(poly)]
            if sp >= 0:
                out.append(p)
            if (sp > 0 and sq < 0) or (sp < 0 and sq > 0):
                t = sp / (sp - sq)
                out.append((p[0] + t * (q[0] - p[0]), p[1] + t * (q[1] - p[1])))
        poly = out
        if len(poly) < 3:
            return 0.0
    ox, oy = poly[0]                                                       # relative to a vertex: no cancellation far from 0
    area = 0.0
    for k in range(1, len(poly) - 1):
        area += (poly[k][0] - ox) * (poly[k + 1][1] - oy) - (poly[k][1] - oy) * (poly[k + 1][0] - ox)
    return abs(area) / 2.0


def clip_iou(a, b):
    o = clip_area(a, b)
    return o / max(float(a[3]) * float(a[4]) + float(b[3]) * float(b[4]) - o, 1e-8)


def exact_matrix(a, b):
    """(area, iou) [len(a), len(b)] float64 by the clip."""
    area = np.array([[clip_area(p, q) for q in b] for p in a], np.float64).reshape(len(a), len(b))
    iou = np.array([[clip_iou(p, q) for q in b] for p in a], np.float64).reshape(len(a), len(b))
    return area, iou


def box(x, y, dx, dy, r, z=0.5, dz=1.5):
    return [x, y, z, dx, dy, dz, r]


SQ45 = 8.0 * (math.sqrt(2.0) - 1.0)
SHIFTS = ((0.0, 0.0), (70.0, -30.0))
# name: box a, box b, expected area, expected IoU (None: not a closed form, area / (sum - area))
CLOSED_FORMS = [
    ("identical", box(0, 0, 3.75, 1.75, 0.5), box(0, 0, 3.75, 1.75, 0.5), 3.75 * 1.75, 1.0),
    ("heading_plus_pi", box(0, 0, 3.75, 1.75, 0.5), box(0, 0, 3.75, 1.75, 0.5 + math.pi), 3.75 * 1.75, 1.0),
    ("square_turned_pi_4", box(0, 0, 2, 2, 0.0), box(0, 0, 2, 2, math.pi / 4), SQ45, SQ45 / (8.0 - SQ45)),
    ("cross_6x1_1x6", box(0, 0, 6, 1, 0.3), box(0, 0, 1, 6, 0.3), 1.0, 1.0 / 11.0),
    ("inside_other_heading", box(0.2, -0.1, 1.0, 0.5, 1.1), box(0, 0, 4, 3, 0.2), 0.5, 0.5 / 12.0),
    ("shared_full_edge", box(0, 0, 2, 2, 0.0), box(2, 0, 2, 2, 0.0), 0.0, 0.0),
    ("inside_sharing_two_edges", box(0.5, 0, 1, 2, 0.0), box(0, 0, 2, 2, 0.0), 2.0, 0.5),
    ("disjoint", box(0, 0, 2, 1, 0.7), box(4, 3, 2, 1, -0.5), 0.0, 0.0),
    ("zero_size_inside", box(0.3, 0.2, 0, 0, 0.5), box(0, 0, 2, 2, 0.0), 0.0, 0.0),
    ("zero_size_both", box(0, 0, 0, 0, 0.0), box(0, 0, 0, 0, 0.0), 0.0, 0.0),
]
# headings outside [-pi, pi] against their reduced angles: equal areas (a, the partner, the same partner reduced)
WRAPPED = [(box(0.3, 0.4, 3, 2, 0.2), box(0, 0, 4, 1.5, 7.5), box(0, 0, 4, 1.5, 7.5 - 2 * math.pi)),
           (box(0.3, 0.4, 3, 2, 0.2), box(0, 0, 4, 1.5, -9.0), box(0, 0, 4, 1.5, -9.0 + 2 * math.pi))]


def shifted(b, shift):
    out = np.array(b, np.float32).reshape(-1, 7).copy()
    out[:, 0] += np.float32(shift[0])
    out[:, 1] += np.float32(shift[1])
    return out


def closed_form_batch(shift):
    """(a [n, 7], b [n, 7], area [n], iou [n]) float32 boxes of CLOSED_FORMS moved by `shift`; pair i is (a[i], b[i])."""
    a = shifted([c[1] for c in CLOSED_FORMS], shift)
    b = shifted([c[2] for c in CLOSED_FORMS], shift)
    return a, b, np.array([c[3] for c in CLOSED_FORMS]), np.array([c[4] for c in CLOSED_FORMS])


# ---- random pairs
PAIR_OFFSETS = (0.0, 70.0, 1000.0)           # metres; the centre sits at (offset, -3 / 7 offset): (70, -30) at 70 m
PAIRS = 256
SEPARATION = 0.05                            # every corner at least this far from the other box's boundary
# Worst error of the oracle (fp32, the reference's algorithm) against the clip at each offset, over the 256 pairs in both argument
# orders, measured on the CPU and rounded up to two digits: offset -> (area in m^2, IoU).  Measured 1.40e-6 / 1.95e-7 at 0 m,
# 3.45e-5 / 4.60e-6 at 70 m and 4.24e-4 / 6.56e-5 at 1000 m (areas up to 14.6 m^2).  CLOSED_FORMS at the origin and at (70, -30)
# stay inside the 0 m and 70 m rows (4.8e-7 / 1.2e-7 and 1.6e-5 / 3.4e-6).  test_center_edges_host.py asserts all of it; the kernels
# are allowed KERNEL_FACTOR times as much (last-place differences of the device sinf, cosf and atan2f).
ORACLE_ERR = {0.0: (1.4e-6, 2.0e-7), 70.0: (3.5e-5, 4.6e-6), 1000.0: (4.3e-4, 6.6e-5)}
KERNEL_FACTOR = 2.0


def boundary_distance(p, b):
    """Distance of point p from the boundary of rectangle b, float64."""
    c, s = math.cos(float(b[6])), math.sin(float(b[6]))
    px, py = p[0] - float(b[0]), p[1] - float(b[1])
    rx, ry = abs(px * c + py * s), abs(-px * s + py * c)
    hx, hy = float(b[3]) / 2, float(b[4]) / 2
    if rx <= hx and ry <= hy:
        return min(hx - rx, hy - ry)
    return math.hypot(max(rx - hx, 0.0), max(ry - hy, 0.0))


def separation(a, b):
    return min(min(boundary_distance(p, b) for p in corners64(a)), min(boundary_distance(p, a) for p in corners64(b)))


def random_pairs(offset):
    """256 pairs (a [256, 7], b [256, 7]) float32 around (offset, -3 / 7 offset): dimensions in [0.5, 5], headings in [-7, 7], the
    partner displaced by about 1 m and 0.6 rad.  Seeded rejection: a candidate is kept when, for the float32 boxes the kernels
    get, every corner of either box is at least SEPARATION from the other's boundary - so neither the 1e-2 inside margin nor the
    proper-crossing rule of the reference algorithm decides an area."""
    rng = np.random.default_rng(7000 + int(offset))
    a, b = [], []
    while len(a) < PAIRS:
        p = np.zeros(7)
        p[0:2] = rng.uniform(-2, 2, 2) + (offset, -3.0 / 7.0 * offset)
        p[2], p[5] = rng.uniform(-1, 1), rng.uniform(1, 2)
        p[3:5] = rng.uniform(0.5, 5.0, 2)
        p[6] = rng.uniform(-7, 7)
        q = p.copy()
        q[0:2] += rng.normal(0, 1.0, 2)
        q[3:5] = rng.uniform(0.5, 5.0, 2)
        q[6] = np.clip(p[6] + rng.normal(0, 0.6), -7, 7)
        p32, q32 = p.astype(np.float32), q.astype(np.float32)
        if separation(p32, q32) >= SEPARATION:
            a.append(p32)
            b.append(q32)
    return np.stack(a), np.stack(b)


# ====================================================================================================== NMS
LATTICE_PITCH, LATTICE_ROW = 3.0, 65
CHAIN_SHIFT, CHAIN_THRESH = 0.6, 0.5
CHAIN_TRIPLES = [(0, 1, 2), (62, 63, 64), (63, 64, 65), (10, 100, 190)]
CHAIN_N = 256


def lattice(n):
    """n axis-aligned 2 x 2 boxes on a 3 m lattice, 65 to a row: no two overlap (or touch)."""
    i = np.arange(n)
    out = np.zeros((n, 7), np.float32)
    out[:, 0], out[:, 1] = (i % LATTICE_ROW) * LATTICE_PITCH, (i // LATTICE_ROW) * LATTICE_PITCH
    out[:, 2], out[:, 3], out[:, 4], out[:, 5] = 0.5, 2.0, 2.0, 1.5
    return out


def late_duplicates():
    """(boxes [4160, 7], keep): boxes 4100..4159 repeat boxes 0..59 (suppression word 64 updated by rows of word 0: the second
    trip of the sweep's `w += 64` loop), box 64 repeats box 63 (across the first word boundary), box 128 repeats box 0."""
    b = lattice(4160)
    b[4100:4160] = b[0:60]
    b[64], b[128] = b[63], b[0]
    dead = set(range(4100, 4160)) | {64, 128}
    return b, np.array([i for i in range(4160) if i not in dead], np.int64)


def chain(triple, n=CHAIN_N):
    """(boxes [n, 7], keep): the lattice with A, B, C at the indices of `triple` moved to a row of their own (y = -10), B and C
    shifted by 0.6 m and 1.2 m from A.  IoU(A, B) = IoU(B, C) = 2.8 / 5.2 > 0.5 > IoU(A, C) = 1.6 / 6.4: A removes B, and C,
    which only B overlaps, stays."""
    b = lattice(n)
    for k, i in enumerate(triple):
        b[i, 0], b[i, 1] = np.float32(CHAIN_SHIFT * k), -10.0
    return b, np.array([i for i in range(n) if i != triple[1]], np.int64)


def aabb_iou(boxes):
    """IoU matrix [n, n] float64 of axis-aligned boxes (heading 0), from the interval overlaps."""
    b = np.asarray(boxes, np.float64)
    lo, hi = b[:, 0:2] - b[:, 3:5] / 2, b[:, 0:2] + b[:, 3:5] / 2
    w = np.clip(np.minimum(hi[:, None], hi[None]) - np.maximum(lo[:, None], lo[None]), 0, None)
    inter = w[..., 0] * w[..., 1]
    area = b[:, 3] * b[:, 4]
    return inter / np.maximum(area[:, None] + area[None] - inter, 1e-8)


def greedy_keep(iou, thresh):
    """Greedy sweep over a score-ordered IoU matrix, from the definition (host cross-check of the constructed keep lists)."""
    alive = np.ones(len(iou), bool)
    keep = []
    for i in range(len(iou)):
        if alive[i]:
            keep.append(i)
            alive[i + 1:] &= ~(iou[i, i + 1:] > thresh)
    return np.array(keep, np.int64)


def mask_words(iou, thresh):
    """The pairwise pass's documented result: word [row, col_block] bit j = IoU(row, 64 col_block + j) > thresh for boxes after
    `row` only, as uint64 [n, ceil(n / 64)]."""
    n = len(iou)
    cb = (n + 63) // 64
    words = np.zeros((n, cb), np.uint64)
    hit = np.triu(iou > thresh, 1)
    for r, c in zip(*np.nonzero(hit)):
        words[r, c // 64] |= np.uint64(1) << np.uint64(c % 64)
    return words
