"""The tables, site sets and fp64 references of tests/spconv_table_cases.py, checked without a GPU: every hand table has the property its
fill promises, every geometric set has the residue classes it is named after (against the CPU oracle's own tables), and the numpy
references agree with the oracle's gather / GEMM / scatter (oracle tolerance 1e-4)."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import spconv_table_cases as C
from tests.test_gpu_parity import CONV_GEOMS


def test_sizes_and_volumes_are_the_ones_asked_for():
    assert C.SIZES == ((1, 129), (129, 1), (7, 33), (33, 17), (300, 257)) and C.K_VOLS == (27, 3)
    assert C.FILLS == ("full", "sparse", "last_only", "empty_offsets", "same_row")
    assert C.ONE_CLASS_ROWS == (1, 33, 129) and C.MIXED_ROWS == (8191, 8192, 8193)


@pytest.mark.parametrize("K", C.K_VOLS)
@pytest.mark.parametrize("n_gather,n_produce", C.SIZES)
def test_hand_tables_have_the_property_of_their_fill(K, n_gather, n_produce):
    for seed, fill in enumerate(C.FILLS):
        t = C.hand_table(K, n_gather, n_produce, fill, seed)
        assert t.dtype == np.int32 and t.shape == (K, n_produce) and t.flags.c_contiguous, fill
        assert t.min() >= -1 and t.max() < n_gather, fill
        assert np.array_equal(t, C.hand_table(K, n_gather, n_produce, fill, seed)), fill      # a function of its arguments
        pairs = (t >= 0).sum(1)
        if fill == "full":
            assert (pairs == n_produce).all()
            assert n_gather == 1 or n_produce * K < 8 or len(np.unique(t)) > 1
        elif fill == "sparse":
            mean = K * n_produce / 64.0      # each entry valid with probability 1 / 64: at most the mean + 6 sigma, never none
            assert 1 <= pairs.sum() <= mean + 6 * np.sqrt(mean) + 1
        elif fill == "last_only":
            assert pairs.sum() == 1 and t[K - 1, n_produce - 1] == n_gather - 1
        elif fill == "empty_offsets":
            empty = C.empty_offsets(K)
            assert set(empty) == {0, K // 2, K - 1}
            assert (pairs[empty] == 0).all() and (np.delete(pairs, empty) == n_produce).all()
        else:
            assert (t == 0).all()


@pytest.mark.parametrize("ks,st,pd", CONV_GEOMS)
def test_class_offsets_partition_the_kernel(ks, st, pd):
    lists = C.class_offsets(ks, st)
    K = int(np.prod(ks))
    assert len(lists) == int(np.prod(st)) and sorted(sum(lists, [])) == list(range(K))
    assert all(lst == sorted(lst) for lst in lists)
    assert sorted(len(lst) for lst in lists) == ([1, 2, 2, 2, 4, 4, 4, 8] if st == (2, 2, 2) else [1, 2])


def _pairs_lie_on_class_offsets(sites, geom):
    ks, st, pd = geom
    shape = C.ONE_CLASS_SHAPE if len(sites) < 1000 else C.MIXED_SHAPE
    assert sites.dtype == np.int32 and len(np.unique(sites, axis=0)) == len(sites)
    assert (sites[:, 0] >= 0).all() and (sites[:, 0] < C.BATCH).all()
    assert all((sites[:, 1 + a] >= 0).all() and (sites[:, 1 + a] < shape[a]).all() for a in range(3))
    _, _, o2i, i2o, cnt = O.rulebook_conv(sites, C.BATCH, list(shape), ks, st, pd)
    assert i2o.shape == (int(np.prod(ks)), len(sites)) and cnt.sum() == (i2o >= 0).sum() == (o2i >= 0).sum() > 0
    cls = C.site_class(sites, st, pd)
    lists = C.class_offsets(ks, st)
    allowed = np.zeros((len(lists), i2o.shape[0]), bool)
    for c, lst in enumerate(lists):
        allowed[c, lst] = True
    assert not ((i2o >= 0) & ~allowed[cls].T).any()
    return cls, i2o


@pytest.mark.parametrize("ks,st,pd", CONV_GEOMS)
def test_one_class_sets_hold_one_class(ks, st, pd):
    geom = (ks, st, pd)
    res = C.residues(st)
    assert len(res) == (8 if st == (2, 2, 2) else 2)
    for c, residue in enumerate(res):
        for n in C.ONE_CLASS_ROWS:
            sites = C.one_class(geom, residue, n)
            assert sites.shape == (n, 4)
            cls, i2o = _pairs_lie_on_class_offsets(sites, geom)
            assert (cls == c).all(), (residue, n)
            for a in range(3):
                assert ((sites[:, 1 + a] + pd[a]) % st[a] == residue[a]).all()
            # only the candidate offsets of the class hold pairs, and an inner site has a pair on every one of them
            lst = C.class_offsets(ks, st)[c]
            assert not (np.delete(i2o, lst, 0) >= 0).any()
            if n > 1:
                assert ((i2o[lst] >= 0).all(0)).any(), (residue, n)


@pytest.mark.parametrize("ks,st,pd", CONV_GEOMS)
def test_mixed_sets_hold_every_class(ks, st, pd):
    for n in C.MIXED_ROWS:
        sites = C.mixed((ks, st, pd), n)
        assert sites.shape == (n, 4)
        cls, _ = _pairs_lie_on_class_offsets(sites, (ks, st, pd))
        assert set(cls.tolist()) == set(range(int(np.prod(st))))


def _operands(nbr, n_gather, cin, cout, seed):
    rng = np.random.default_rng(seed)
    K, n_produce = nbr.shape
    feat = rng.standard_normal((n_gather, cin)).astype(np.float32)
    w = (rng.standard_normal((cout,) + C.KSHAPE[K] + (cin,)) / np.sqrt(K * cin)).astype(np.float32)
    bias = rng.standard_normal(cout).astype(np.float32)
    g = rng.standard_normal((n_produce, cout)).astype(np.float32)
    return feat, w, bias, g


def _references_agree(nbr, n_gather, cin, cout, seed):
    """nbr [K, n_produce] into n_gather rows: the forward and the weight gradient over it, and a data gradient that gathers rows of cout
    channels through the same table (offsets in table order and reversed)."""
    feat, w, bias, g = _operands(nbr, n_gather, cin, cout, seed)
    tol = dict(rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(C.ref_fwd(feat, w, nbr, bias), O.spconv_fwd(feat, w, nbr, bias), **tol)
    np.testing.assert_allclose(C.ref_fwd(feat, w, nbr), O.spconv_fwd(feat, w, nbr), **tol)
    np.testing.assert_allclose(C.ref_wgrad(feat, g, nbr, w.shape), O.spconv_wgrad(feat, g, nbr, w.shape), **tol)
    gg = np.random.default_rng(seed + 1).standard_normal((n_gather, cout)).astype(np.float32)      # the data gradient gathers n_gather rows of cout
    for flip in (False, True):
        np.testing.assert_allclose(C.ref_dgrad(gg, w, nbr, flip), O.spconv_dgrad(gg, w, nbr, flip_k=flip), **tol)


@pytest.mark.parametrize("K,size,fill", [(27, (300, 257), "full"), (3, (33, 17), "sparse"), (27, (7, 33), "empty_offsets")])
def test_references_agree_with_the_oracle_on_hand_tables(K, size, fill):
    _references_agree(C.hand_table(K, size[0], size[1], fill, 5), size[0], 6, 10, seed=K + size[0])


def test_references_agree_with_the_oracle_on_a_geometric_table():
    ks, st, pd = CONV_GEOMS[1]
    sites = C.one_class((ks, st, pd), (0, 0, 0), 129)
    _, _, o2i, i2o, _ = O.rulebook_conv(sites, C.BATCH, list(C.ONE_CLASS_SHAPE), ks, st, pd)
    _references_agree(o2i, len(sites), 6, 10, seed=1)
    _references_agree(i2o, o2i.shape[1], 10, 6, seed=2)
