"""Coordinate sets, case tables and a plain reference for the grid index and the rulebooks of toda_amd/csrc/rulebook.hip, shared by
test_rulebook_host.py (no GPU) and test_gpu_rulebook_edges.py.

The reference is written from the definition of the two operations and looks every neighbour up in a sorted-key dictionary of the
INPUT set, output stationary: an output cell is a site when one input site lies in its window, and the input behind tap k of output
o is the site at o * stride - pad + k.  oracle/toda_oracle.c goes the other way round (input stationary, a hash of the output set),
so the two share no formula beyond the output-shape one; test_rulebook_host.py checks that they agree on every case of this file."""
import numpy as np

from tests import helpers as H


# ---------------------------------------------------------------------------------------------- keys and row orders
def lin_keys(idx, shape):
    """((b*D+z)*H+y)*W+x as int64"""
    i = np.asarray(idx, np.int64).reshape(-1, 4)
    return ((i[:, 0] * shape[0] + i[:, 1]) * shape[1] + i[:, 2]) * shape[2] + i[:, 3]


def canonical(idx, shape):
    idx = np.asarray(idx, np.int32).reshape(-1, 4)
    return np.ascontiguousarray(idx[np.argsort(lin_keys(idx, shape), kind="stable")])


def both_orders(idx, shape, seed):
    """(canonical, shuffled): the same unique rows in ascending key order and in a seeded random order"""
    canon = canonical(np.unique(np.asarray(idx, np.int32).reshape(-1, 4), axis=0), shape)
    perm = np.random.default_rng(seed).permutation(len(canon))
    if len(canon) > 1 and np.array_equal(perm, np.arange(len(canon))):
        perm = perm[::-1]
    return canon, np.ascontiguousarray(canon[perm])


def in_lattice(idx, batch, shape):
    i = np.asarray(idx, np.int64).reshape(-1, 4)
    return (i[:, 0] >= 0) & (i[:, 0] < batch) & np.all((i[:, 1:] >= 0) & (i[:, 1:] < np.asarray(shape, np.int64)), axis=1)


# ---------------------------------------------------------------------------------------------- coordinate sets
def clustered(batch, shape, seed, n_per_batch=None):
    if n_per_batch is None:
        n_per_batch = int(min(600, max(2, int(np.prod(shape)) // 5)))
    idx, _ = H.clustered_sparse(batch, list(shape), n_per_batch, 1, seed=seed)
    return both_orders(idx, shape, seed + 1)


def full(batch, shape, seed=0):
    g = np.stack(np.meshgrid(np.arange(batch), np.arange(shape[0]), np.arange(shape[1]), np.arange(shape[2]), indexing="ij"), -1)
    return both_orders(g.reshape(-1, 4), shape, seed + 1)


def first_cell(batch, shape, seed=0):
    return both_orders([[0, 0, 0, 0]], shape, seed)


def last_cell(batch, shape, seed=0):
    return both_orders([[batch - 1, shape[0] - 1, shape[1] - 1, shape[2] - 1]], shape, seed)


def no_site(batch, shape, seed=0):
    return both_orders(np.zeros((0, 4), np.int32), shape, seed)


def one_sample_empty(batch, shape, seed, empty=None):
    """clustered, but batch sample `empty` (default: the middle one) holds no site"""
    canon, _ = clustered(batch, shape, seed)
    empty = batch // 2 if empty is None else empty
    return both_orders(canon[canon[:, 0] != empty], shape, seed + 2)


def faces(batch, shape, seed=0):
    """every cell on a face of the lattice (so all edges and corners), nothing inside"""
    canon, _ = full(batch, shape)
    hi = np.asarray(shape, np.int32) - 1
    on = np.any((canon[:, 1:] == 0) | (canon[:, 1:] == hi), axis=1)
    return both_orders(canon[on], shape, seed + 3)


def clusters(batch, shape, centres, n_each, seed, spread=(0.8, 5.0, 30.0)):
    """a few hundred sites around each (b, z, y, x) centre, clipped to the lattice; the centres themselves are sites"""
    rng = np.random.default_rng(seed)
    hi = np.asarray(shape, np.int64) - 1
    rows = []
    for c in centres:
        c = np.asarray(c, np.int64)
        d = np.rint(rng.normal(0.0, 1.0, (n_each, 3)) * np.asarray(spread)).astype(np.int64)
        p = np.clip(c[1:] + d, 0, hi)
        rows.append(np.concatenate([np.full((n_each, 1), c[0]), p], 1))
        rows.append(c[None])
    return both_orders(np.concatenate(rows), shape, seed + 4)


# ---------------------------------------------------------------------------------------------- the reference
def conv_out_shape(shape, ks, st, pd):
    return [(int(s) + 2 * int(p) - int(k)) // int(t) + 1 for s, k, t, p in zip(shape, ks, st, pd)]


class SiteDict:
    """coordinate -> row of a coordinate list, a dictionary kept as sorted keys; rows outside the lattice are not in it"""

    def __init__(self, idx, batch, shape):
        self.batch, self.shape = int(batch), [int(v) for v in shape]
        idx = np.asarray(idx, np.int64).reshape(-1, 4)
        rows = np.flatnonzero(in_lattice(idx, batch, shape))
        keys = lin_keys(idx[rows], shape)
        order = np.argsort(keys, kind="stable")
        self.keys, self.rows = keys[order], rows[order]
        assert len(np.unique(self.keys)) == len(self.keys), "coordinates must be unique"

    def row(self, coords):
        """row of every (b, z, y, x) in `coords`, -1 where the cell is outside the lattice or holds no site"""
        c = np.asarray(coords, np.int64).reshape(-1, 4)
        ok = in_lattice(c, self.batch, self.shape)
        out = np.full(len(c), -1, np.int64)
        if len(self.keys) and ok.any():
            k = lin_keys(c[ok], self.shape)
            pos = np.minimum(np.searchsorted(self.keys, k), len(self.keys) - 1)
            out[ok] = np.where(self.keys[pos] == k, self.rows[pos], -1)
        return out


def taps(ks):
    """kernel offsets (kz, ky, kx) in table order k = (kz * KY + ky) * KX + kx"""
    return [(kz, ky, kx) for kz in range(ks[0]) for ky in range(ks[1]) for kx in range(ks[2])]


def subm_reference(idx, batch, shape, ks, dil):
    """(nbr [K, n] int32, counts [K] int32): nbr[k, o] = row of the site at coords[o] + (tap - ks // 2) * dilation, or -1"""
    idx = np.asarray(idx, np.int64).reshape(-1, 4)
    d = SiteDict(idx, batch, shape)
    live = in_lattice(idx, batch, shape)
    nbr = np.full((len(taps(ks)), len(idx)), -1, np.int64)
    for k, tap in enumerate(taps(ks)):
        q = idx.copy()
        for a in range(3):
            q[:, 1 + a] += (tap[a] - ks[a] // 2) * dil[a]
        nbr[k] = np.where(live, d.row(q), -1)
    return nbr.astype(np.int32), (nbr >= 0).sum(1).astype(np.int32)


def conv_reference(idx, batch, shape, ks, st, pd):
    """(out_indices [n_out, 4] int32 ascending, out_shape, o2i [K, n_out], i2o [K, n_in], counts [K]) of a strided convolution"""
    idx = np.asarray(idx, np.int64).reshape(-1, 4)
    n_in = len(idx)
    out_shape = conv_out_shape(shape, ks, st, pd)
    K = len(taps(ks))
    assert all(v >= 1 for v in out_shape), out_shape
    live = idx[in_lattice(idx, batch, shape)]
    # candidates: per axis the outputs o whose window [o * s - p, o * s - p + k) holds the input coordinate
    per_axis = []
    for a in range(3):
        c = live[:, 1 + a]
        top = (c + pd[a]) // st[a]
        cand = np.stack([top - j for j in range(-(-ks[a] // st[a]))], 1)
        ok = (cand >= 0) & (cand < out_shape[a]) & (cand * st[a] - pd[a] + ks[a] - 1 >= c[:, None]) & (cand * st[a] - pd[a] <= c[:, None])
        per_axis.append((cand, ok))
    rows = []
    for jz in range(per_axis[0][0].shape[1]):
        for jy in range(per_axis[1][0].shape[1]):
            for jx in range(per_axis[2][0].shape[1]):
                ok = per_axis[0][1][:, jz] & per_axis[1][1][:, jy] & per_axis[2][1][:, jx]
                rows.append(np.stack([live[ok, 0], per_axis[0][0][ok, jz], per_axis[1][0][ok, jy], per_axis[2][0][ok, jx]], 1))
    out = np.unique(np.concatenate(rows), axis=0) if rows and n_in else np.zeros((0, 4), np.int64)
    out = out[np.argsort(lin_keys(out, out_shape), kind="stable")]
    n_out = len(out)
    d = SiteDict(idx, batch, shape)
    o2i = np.full((K, n_out), -1, np.int64)
    i2o = np.full((K, n_in), -1, np.int64)
    for k, tap in enumerate(taps(ks)):
        q = out.copy()
        for a in range(3):
            q[:, 1 + a] = out[:, 1 + a] * st[a] - pd[a] + tap[a]
        o2i[k] = d.row(q)
        hit = np.flatnonzero(o2i[k] >= 0)
        i2o[k, o2i[k, hit]] = hit
    assert (o2i >= 0).any(0).all(), "an output without an input"
    return out.astype(np.int32), out_shape, o2i.astype(np.int32), i2o.astype(np.int32), (o2i >= 0).sum(1).astype(np.int32)


# ---------------------------------------------------------------------------------------------- the grid index buffer
class Layout:
    """Byte layout of a grid-index buffer (gi_layout of grid_index.cuh): {bits, rank of the word's first cell} pairs, the scan's
    partial sums, one total, one byte per lattice row (b, z, y); every region starts on a multiple of 256 bytes."""

    def __init__(self, batch, shape):
        up = lambda v: -(-v // 256) * 256      # noqa: E731
        self.bits = int(batch) * int(shape[0]) * int(shape[1]) * int(shape[2])
        self.cells = -(-self.bits // 32)
        self.rows = int(batch) * int(shape[0]) * int(shape[1])
        self.o_cells = 0
        self.o_part = up(self.cells * 8)
        self.o_total = self.o_part + up((-(-self.cells // 256) + 1) * 4)
        self.o_rows = self.o_total + 256
        self.bytes = self.o_rows + up(self.rows)


def popcount32(a):
    a = np.ascontiguousarray(a, dtype=np.uint32)
    return np.unpackbits(a.view(np.uint8).reshape(-1, 4), axis=1).sum(1).astype(np.int64)


def bitmap_words(idx, batch, shape):
    """the occupancy words of a coordinate list (bit l & 31 of word l >> 5), uint32 [cells]"""
    lay = Layout(batch, shape)
    idx = np.asarray(idx, np.int64).reshape(-1, 4)
    keys = lin_keys(idx[in_lattice(idx, batch, shape)], shape)
    words = np.zeros(lay.cells, np.uint32)
    np.bitwise_or.at(words, keys >> 5, (np.uint32(1) << (keys & 31).astype(np.uint32)))
    return words


def canonical_cells(idx, batch, shape):
    """[cells, 2] uint32: {occupancy word, number of sites in all earlier words}"""
    words = bitmap_words(idx, batch, shape)
    pc = popcount32(words)
    return np.stack([words, (np.cumsum(pc) - pc).astype(np.uint32)], 1)


def row_bytes(idx, batch, shape):
    """one byte per lattice row (b, z, y): 1 where the row holds a site"""
    idx = np.asarray(idx, np.int64).reshape(-1, 4)
    idx = idx[in_lattice(idx, batch, shape)]
    out = np.zeros(Layout(batch, shape).rows, np.uint8)
    out[(idx[:, 0] * shape[0] + idx[:, 1]) * shape[1] + idx[:, 2]] = 1
    return out


def ranks(cells, keys):
    """rank of every key through a [cells, 2] {bits, first rank} array, -1 where the bit is not set (gi_rank)"""
    keys = np.asarray(keys, np.int64)
    w, b = cells[keys >> 5, 0].astype(np.uint32), (keys & 31).astype(np.uint32)
    below = w & ((np.uint32(1) << b) - np.uint32(1))
    r = cells[keys >> 5, 1].astype(np.int64) + popcount32(below)
    return np.where((w >> b) & np.uint32(1), r, -1)


# ---------------------------------------------------------------------------------------------- case tables
# (kernel, stride, padding) of the strided convolutions
STRIDED_GEOMS = [
    ((2, 2, 2), (2, 2, 2), (0, 0, 0)),
    ((3, 3, 3), (1, 1, 1), (1, 1, 1)),
    ((3, 3, 3), (3, 3, 3), (1, 1, 1)),
    ((1, 3, 3), (1, 2, 2), (0, 1, 1)),
    ((4, 4, 4), (2, 2, 2), (1, 1, 1)),      # K = 64, the limit
    ((1, 1, 9), (1, 1, 1), (0, 0, 4)),      # ks[2] > 8: the per-bit arm of the output-set kernel
    ((1, 1, 4), (1, 1, 4), (0, 0, 0)),      # 31 * 4 + 4 = 128 window bits: the widest x stride toda_gridindex_from_bitmap takes
    ((1, 1, 8), (1, 1, 2), (0, 0, 3)),      # the widest kernel of the shift-OR arm
    ((3, 1, 1), (2, 1, 1), (0, 0, 0)),      # VoxelBackBone8x's last down-sampling layer: the <3, 1, 1> table kernels
]
# (shape, batch)
LATTICES = [
    ((5, 9, 11), 3),
    ((7, 33, 65), 2),
    ((3, 4, 31), 2),
    ((2, 3, 1), 2),       # W = 1
    ((1, 1, 20), 1),      # the whole lattice in one word
    ((4, 6, 64), 1),
]
# the only combinations left out: an axis smaller than its kernel minus twice the padding leaves no output cell.  (geometry, lattice)
EMPTY_OUTPUT = [(0, 3), (0, 4), (4, 3), (4, 4), (6, 3), (7, 3), (8, 3), (8, 4)]
STRIDED_CASES = [(g, l) for g in range(len(STRIDED_GEOMS)) for l in range(len(LATTICES)) if (g, l) not in EMPTY_OUTPUT]


def geom_id(g):
    return "k%d%d%d-s%d%d%d-p%d%d%d" % tuple(v for t in STRIDED_GEOMS[g] for v in t)


def lattice_id(l):
    (d, h, w), b = LATTICES[l]
    return "%dx%dx%dx%d" % (d, h, w, b)


def strided_sites(l):
    shape, batch = LATTICES[l]
    return clustered(batch, shape, seed=100 + l)


# the coordinate sets of the occupancy tests: name -> (batch, shape, (canonical, shuffled))
def occupancy_sets():
    return {
        "full-3x4x33x2": (2, (3, 4, 33), full(2, (3, 4, 33))),
        "full-2x2x64x1": (1, (2, 2, 64), full(1, (2, 2, 64))),
        "first-cell": (2, (3, 4, 33), first_cell(2, (3, 4, 33))),
        "last-cell": (2, (3, 4, 33), last_cell(2, (3, 4, 33))),
        "no-site": (2, (3, 4, 33), no_site(2, (3, 4, 33))),
        "sample-1-of-3-empty": (3, (5, 9, 11), one_sample_empty(3, (5, 9, 11), seed=31)),
        "sample-0-of-2-empty": (2, (3, 4, 31), one_sample_empty(2, (3, 4, 31), seed=32, empty=0)),
        "faces-7x9x64x1": (1, (7, 9, 64), faces(1, (7, 9, 64))),
        "faces-3x4x33x2": (2, (3, 4, 33), faces(2, (3, 4, 33))),
    }


OCCUPANCY_NAMES = ["full-3x4x33x2", "full-2x2x64x1", "first-cell", "last-cell", "no-site", "sample-1-of-3-empty", "sample-0-of-2-empty",
                   "faces-7x9x64x1", "faces-3x4x33x2"]
SUBM_KERNELS = [((3, 3, 3), (1, 1, 1)), ((5, 5, 1), (1, 2, 3)), ((3, 3, 7), (1, 2, 3))]     # (kernel, dilation); 3x3x3 has its own kernel
OCC_CONV = ((3, 3, 3), (2, 2, 2), (1, 1, 1))

# the scan's carry loop: more than 256 tiles of 2048 words
CARRY_SHAPE, CARRY_BATCH = (5, 1900, 1800), 1
CARRY_CONV = ((3, 3, 3), (1, 1, 1), (1, 1, 1))


def carry_sites():
    d, h, w = CARRY_SHAPE
    return clusters(CARRY_BATCH, CARRY_SHAPE, [(0, 0, 1, 5), (0, 2, 950, 900), (0, 4, 1897, 1790), (0, 0, 0, 0), (0, d - 1, h - 1, w - 1)],
                    900, seed=41)


# 64-bit coordinate arithmetic: 2^31 cells is the smallest lattice that reaches it
BIG_SHAPE, BIG_BATCH = (9, 15450, 15450), 1
BIG_CONV = ((3, 3, 3), (1, 1, 1), (1, 1, 1))


def coord_of(key, shape):
    key, x = divmod(int(key), shape[2])
    key, y = divmod(key, shape[1])
    b, z = divmod(key, shape[0])
    return (b, z, y, x)


def big_sites():
    d, h, w = BIG_SHAPE
    at = coord_of(2 ** 31, BIG_SHAPE)
    canon, _ = clusters(BIG_BATCH, BIG_SHAPE, [(0, 0, 1, 6), at, (0, d - 1, h - 1, w // 2), (0, 0, 0, 0), (0, d - 1, h - 1, w - 1)], 800, seed=43)
    extra = [coord_of(2 ** 31 + o, BIG_SHAPE) for o in (-33, -32, -1, 0, 1, 31, 32)]
    return both_orders(np.concatenate([canon, np.asarray(extra, np.int32)]), BIG_SHAPE, seed=44)


# what the library must refuse: (entry point, kernel, stride or dilation, padding)
REFUSED_SUBM = [((5, 5, 3), "volume"), ((2, 3, 3), "odd")]
REFUSED_CONV = ((5, 5, 3), (1, 1, 1), (2, 2, 1))
TOO_WIDE = ((1, 1, 5), (1, 1, 4), (0, 0, 0))       # 31 * 4 + 5 = 129 window bits: refused by from_bitmap, taken by from_conv
