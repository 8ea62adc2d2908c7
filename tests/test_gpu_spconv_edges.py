"""Row-count edges of the sparse gather-GEMMs and weight gradients (csrc/spconv.hip, csrc/spconv_split.cuh; reference call sites
pcdet/models/backbones_3d/spconv_backbone.py:77-125) that the other sparse-conv tests, all at 1100 rows or more, do not reach:
  1 row     one live lane in one tile, three waves of the only workgroup wholly past the end
  33 rows   one over a wave's two 16-row tiles: the second wave has one live row
  129 rows  one over a workgroup's 128 rows: the second workgroup has one live row
for the weight gradient these are queues that never fill a round (1), a ragged tail (33) and the third 64-row batch of a chunk (129).
Every result is checked against an fp64 evaluation of the same sums on the device (test_gpu_split.exact_sums / exact_wgrad) at the
oracle tolerance of test_gpu_parity (1e-4), under both matrix paths, and a second call must give the same bits."""
import functools

import numpy as np
import pytest
import torch

from tests import helpers as H
from tests.test_gpu_split import dev, exact_sums, exact_wgrad, paths  # noqa: F401  (paths is a fixture)

pytestmark = pytest.mark.gpu

SHAPE, BATCH = [9, 40, 44], 2
PAIRS = [(16, 16), (24, 48), (64, 64), (128, 128)]
ROWS = [1, 33, 129]


@functools.lru_cache(maxsize=None)
def _sites():
    idx, _ = H.clustered_sparse(BATCH, SHAPE, 200, 1, seed=21)
    assert len(idx) >= max(ROWS)
    return idx


def _table(ops, n):
    """A submanifold table over the first n sites of one clustered set (K = 27)."""
    return ops.build_subm_rulebook(dev(_sites()[:n]), BATCH, SHAPE)[0]


def _operands(cin, cout, n):
    rng = np.random.default_rng(1000 * cin + 10 * cout + n)
    feat = rng.standard_normal((n, cin)).astype(np.float32)
    w = (rng.standard_normal((cout, 3, 3, 3, cin)) / np.sqrt(27 * cin)).astype(np.float32)
    bias = rng.standard_normal(cout).astype(np.float32)
    g = rng.standard_normal((n, cout)).astype(np.float32)
    return dev(feat), dev(w), dev(bias), dev(g)


@pytest.mark.parametrize("n", ROWS)
@pytest.mark.parametrize("cin,cout", PAIRS)
def test_forward_dgrad_wgrad_at_row_edges(cin, cout, n, paths):
    ops = paths
    rb = _table(ops, n)
    assert rb.n_out == n
    x, w, b, g = _operands(cin, cout, n)
    ref_f = exact_sums(x, w, rb.nbr_fwd, False, False) + b.double()
    ref_d = exact_sums(g, w, rb.nbr_bwd, True, True)
    ref_w = exact_wgrad(x, g, rb.nbr_fwd, cout, cin)
    scale_w = max(float(ref_w.pow(2).mean().sqrt()), 1.0)

    def run():
        return (ops.gather_gemm(x, ops.pack_weight(w, False, False), rb.nbr_fwd, cout, b),
                ops.gather_gemm(g, ops.pack_weight(w, True, True), rb.nbr_bwd, cin),
                ops.wgrad(x, g, rb.nbr_fwd, tuple(w.shape)))

    for mm in ("native", "split"):
        ops.set_matrix_path(mm)
        f, d, dw = run()
        assert f.shape == (n, cout) and d.shape == (n, cin)
        np.testing.assert_allclose(f.cpu().numpy(), ref_f.cpu().numpy(), rtol=1e-4, atol=1e-4, err_msg=mm)
        np.testing.assert_allclose(d.cpu().numpy(), ref_d.cpu().numpy(), rtol=1e-4, atol=1e-4, err_msg=mm)
        np.testing.assert_allclose(dw.reshape(cout, 27, cin).cpu().numpy(), ref_w.cpu().numpy(), rtol=1e-4, atol=1e-4 * scale_w, err_msg=mm)
        again = run()
        assert all(torch.equal(p, q) for p, q in zip(again, (f, d, dw))), mm      # no atomics: bit-reproducible


def test_epilogue_moments_with_one_live_row_in_the_last_workgroup(paths):
    """64 -> 64 at 129 rows: the second workgroup holds one live row and three waves wholly past the end, which still take part in the
    epilogue's barrier.  The moments equal an fp64 pass over the stored output (tolerances of test_gpu_parity's
    test_conv_epilogue_bn_moments_equal_a_pass_over_the_output), folded or left as per-workgroup partials."""
    ops = paths
    cin = cout = 64
    n = 129
    rb = _table(ops, n)
    x, w, b, _ = _operands(cin, cout, n)
    for mm in ("native", "split"):
        ops.set_matrix_path(mm)
        assert ops.gather_gemm_stats_supported(cin, cout)
        wp = ops.pack_weight(w, False, False)
        out, sums = ops.gather_gemm_with_stats(x, wp, rb.nbr_fwd, cout, b)
        assert torch.equal(out, ops.gather_gemm(x, wp, rb.nbr_fwd, cout, b)), mm
        ref = out.double()
        want = torch.cat([ref.sum(0), (ref * ref).sum(0)]).cpu().numpy()
        np.testing.assert_allclose(sums[:2 * cout].cpu().numpy(), want, rtol=1e-5, atol=1e-3, err_msg=mm)
        out_p, part, blocks = ops.gather_gemm_with_stats(x, wp, rb.nbr_fwd, cout, b, partials=True)
        assert blocks == 2 and torch.equal(out_p, out), mm
        folded = part[2 * cout:2 * cout * (1 + blocks)].view(2 * cout, blocks).sum(1)
        np.testing.assert_allclose(folded.cpu().numpy(), want, rtol=1e-5, atol=1e-3, err_msg=mm)
