"""Tables and site sets for the sparse-conv kernel tests (tests/test_spconv_tables_host.py, tests/test_gpu_spconv_tables.py), numpy only.

The gather-GEMMs and weight gradients of csrc/spconv.hip / csrc/spconv_split.cuh take any table [K, produced rows] whose entries lie
in [-1, gathered rows): hand_table builds such tables with the two row counts DIFFERENT (as in a strided convolution and its data
gradient, or an inverse convolution), so that a kernel's row clamp (produced rows - 1), its buffer size (gathered rows) and its store
bound cannot stand in for one another.  one_class / mixed are site sets for the class-sorted data gradient of the strided geometries of
test_gpu_parity.CONV_GEOMS; site_class / class_offsets restate toda_rulebook_class_order's class and the candidate lists of
toda_spconv_gather_gemm_classed; ref_fwd / ref_dgrad / ref_wgrad are fp64 evaluations of the three contractions over any table."""
import functools

import numpy as np

FILLS = ("full", "sparse", "last_only", "empty_offsets", "same_row")
SIZES = ((1, 129), (129, 1), (7, 33), (33, 17), (300, 257))      # (gathered rows, produced rows)
K_VOLS = (27, 3)
KSHAPE = {27: (3, 3, 3), 3: (3, 1, 1)}
ONE_CLASS_ROWS = (1, 33, 129)
MIXED_ROWS = (8191, 8192, 8193)      # toda_rulebook_class_order sorts inside blocks of 8192 rows
ONE_CLASS_SHAPE, MIXED_SHAPE, BATCH = (11, 48, 40), (21, 96, 88), 2


def empty_offsets(K):
    return sorted({0, K // 2, K - 1})


def hand_table(K, n_gather, n_produce, fill, seed):
    """int32 [K, n_produce], entries in [-1, n_gather)."""
    rng = np.random.default_rng(seed)
    full = rng.integers(0, n_gather, (K, n_produce)).astype(np.int32)
    if fill == "full":
        t = full
    elif fill == "sparse":
        keep = rng.random((K, n_produce)) < 1.0 / 64
        if not keep.any():
            keep[K // 2, n_produce // 2] = True
        t = np.where(keep, full, -1).astype(np.int32)
    elif fill == "last_only":
        t = np.full((K, n_produce), -1, np.int32)
        t[K - 1, n_produce - 1] = n_gather - 1
    elif fill == "empty_offsets":
        t = full
        t[empty_offsets(K)] = -1
    elif fill == "same_row":
        t = np.zeros((K, n_produce), np.int32)
    else:
        raise ValueError(fill)
    t.setflags(write=False)
    return t


# ---- residue classes of a strided convolution --------------------------------------------------------------------------------------
def site_class(coords, stride, padding):
    """Class of every input site (b, z, y, x): ((z + pz) mod sz, (y + py) mod sy, (x + px) mod sx) as one number, z slowest."""
    c = np.asarray(coords, np.int64)
    rz, ry, rx = ((c[:, 1 + a] + padding[a]) % stride[a] for a in range(3))
    return ((rz * stride[1] + ry) * stride[2] + rx).astype(np.int64)


def residues(stride):
    """The residue triple of every class, in class order."""
    return [(rz, ry, rx) for rz in range(stride[0]) for ry in range(stride[1]) for rx in range(stride[2])]


def class_offsets(ksize, stride):
    """Per class the kernel offsets (index (kz ky + ky) kx + kx of the table) an input site of that class can have a pair on:
    out = (in + pad - k) / stride is whole only for k = in + pad (mod stride) on every axis.  Ascending."""
    lists = []
    for res in residues(stride):
        ks = [(kz * ksize[1] + ky) * ksize[2] + kx for kz in range(ksize[0]) for ky in range(ksize[1]) for kx in range(ksize[2])
              if (kz % stride[0], ky % stride[1], kx % stride[2]) == res]
        lists.append(ks)
    return lists


def _nearest(cells, n, rng, n_centres):
    """The n cells (rows b, z, y, x) nearest to n_centres random cells (z distances weigh four times: flat clusters), ties jittered."""
    hi = cells[:, 1:].max(0)
    inner = cells[((cells[:, 1:] >= np.minimum(1, hi)) & (cells[:, 1:] <= np.maximum(hi - 1, 0))).all(1)]      # centres off the lattice's faces
    centres = inner[rng.choice(len(inner), n_centres, replace=False)].astype(np.float64)
    best = np.full(len(cells), np.inf)
    for c in centres:
        d = cells.astype(np.float64) - c
        d2 = 16.0 * d[:, 1] ** 2 + d[:, 2] ** 2 + d[:, 3] ** 2 + 1e6 * (d[:, 0] != 0)
        best = np.minimum(best, d2)
    pick = np.argsort(best + 2.0 * rng.random(len(cells)), kind="stable")[:n]
    out = cells[pick][rng.permutation(n)].astype(np.int32)
    assert len(out) == n and len(np.unique(out, axis=0)) == n
    out.setflags(write=False)
    return out


def _lattice(batch, dims):
    b, z, y, x = np.meshgrid(np.arange(batch), np.arange(dims[0]), np.arange(dims[1]), np.arange(dims[2]), indexing="ij")
    return np.stack([b.ravel(), z.ravel(), y.ravel(), x.ravel()], 1)


@functools.lru_cache(maxsize=None)
def one_class(geom, residue, n):
    """n clustered input sites (int32 [n, 4], shuffled) of ONE_CLASS_SHAPE whose (coordinate + padding) mod stride is `residue`."""
    ks, st, pd = geom
    first = [(residue[a] - pd[a]) % st[a] for a in range(3)]
    dims = [len(range(first[a], ONE_CLASS_SHAPE[a], st[a])) for a in range(3)]
    rng = np.random.default_rng(7000 + 100 * site_class(np.array([[0] + first]), st, pd)[0] + n + 13 * sum(pd))
    q = _nearest(_lattice(BATCH, dims), n, rng, 1).astype(np.int64)
    sites = q.copy()
    for a in range(3):
        sites[:, 1 + a] = first[a] + st[a] * q[:, 1 + a]
    sites = sites.astype(np.int32)
    assert all((sites[:, 1 + a] >= 0).all() and (sites[:, 1 + a] < ONE_CLASS_SHAPE[a]).all() for a in range(3))
    sites.setflags(write=False)
    return sites


@functools.lru_cache(maxsize=None)
def clustered(n):
    """n adjacent sites of ONE_CLASS_SHAPE (int32 [n, 4], shuffled), classes as they come."""
    return _nearest(_lattice(BATCH, ONE_CLASS_SHAPE), n, np.random.default_rng(500 + n), 1)


@functools.lru_cache(maxsize=None)
def mixed(geom, n):
    """n clustered input sites (int32 [n, 4], shuffled) of MIXED_SHAPE around a few centres; every class of the geometry occurs."""
    ks, st, pd = geom
    rng = np.random.default_rng(9000 + n + 13 * sum(pd) + 101 * sum(st))
    sites = _nearest(_lattice(BATCH, MIXED_SHAPE), n, rng, 6)
    assert len(np.unique(site_class(sites, st, pd))) == st[0] * st[1] * st[2]
    return sites


# ---- fp64 references over any table ------------------------------------------------------------------------------------------------
def _rows(x, ids):
    """x[ids] in fp64, zero rows where ids < 0."""
    x64 = np.concatenate([np.asarray(x, np.float64), np.zeros((1, x.shape[1]))], 0)
    return x64[np.where(ids >= 0, ids, x.shape[0])]


def ref_fwd(feat, w, nbr, bias=None):
    """out[o] = bias + sum_k W_k feat[nbr[k, o]];  w [cout, kz, ky, kx, cin], nbr [K, n_out]."""
    K, n_out = nbr.shape
    cout, cin = w.shape[0], w.shape[-1]
    wk = np.asarray(w, np.float64).reshape(cout, K, cin)
    out = np.zeros((n_out, cout)) + (0.0 if bias is None else np.asarray(bias, np.float64))
    for k in range(K):
        out += _rows(feat, nbr[k]) @ wk[:, k, :].T
    return out


def ref_dgrad(dout, w, nbr_i2o, flip_k):
    """din[i] = sum_k W_kk^T dout[nbr_i2o[k, i]], kk = K - 1 - k when flip_k (a submanifold layer's forward table read backwards)."""
    K, n_in = nbr_i2o.shape
    cout, cin = w.shape[0], w.shape[-1]
    wk = np.asarray(w, np.float64).reshape(cout, K, cin)
    din = np.zeros((n_in, cin))
    for k in range(K):
        din += _rows(dout, nbr_i2o[k]) @ wk[:, K - 1 - k if flip_k else k, :]
    return din


def ref_wgrad(feat, dout, nbr, wshape):
    """dw[co, k, ci] = sum_o dout[o, co] feat[nbr[k, o], ci], in the shape of the weight."""
    K = nbr.shape[0]
    cout, cin = wshape[0], wshape[-1]
    dw = np.zeros((cout, K, cin))
    g64 = np.asarray(dout, np.float64)
    for k in range(K):
        dw[:, k, :] = g64.T @ _rows(feat, nbr[k])
    return dw.reshape(wshape)
