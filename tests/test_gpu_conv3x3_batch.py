"""The work around the dense Winograd 3x3 layers (toda_amd/csrc/conv2d.hip): the filter transforms of a stack in one launch
(toda_conv3x3_transform_weight_batch + the operand cache of ops.conv3x3_prepack) and the weight gradient's fold + G^T . G in one
kernel.  Both are bit-identical to what they replace, so every comparison here is torch.equal: the batch against the per-layer
entry point, the fused fold against the two-kernel route it replaced (TODA_WGRAD_FOLD=pair, same process, same slabs)."""
import os

import pytest
import torch

from tests import helpers as H

pytestmark = pytest.mark.gpu


def _stack(seed=0):
    """(cout, cin) = (32, 32), (64, 32), (32, 64); on an input without a gradient the first layer wants the forward operand only
    (mode 0), the two behind it both operands (mode 2)."""
    torch.manual_seed(seed)
    return torch.nn.Sequential(torch.nn.Conv2d(32, 32, 3, padding=1, bias=False), torch.nn.ReLU(),
                               torch.nn.ZeroPad2d(1), torch.nn.Conv2d(32, 64, 3, padding=0, bias=False),
                               torch.nn.Sequential(torch.nn.Conv2d(64, 32, 3, padding=1))).cuda()


def _convs(seq):
    return [m for m in seq.modules() if type(m) is torch.nn.Conv2d]


def test_batched_filter_transform_equals_the_per_layer_entry_point():
    from toda_amd import ops

    g = torch.Generator().manual_seed(1)
    ws = [torch.randn((co, ci, 3, 3), generator=g).cuda() for co, ci in ((32, 32), (64, 32), (32, 64))]
    modes = [0, 2, 2]
    with H.abi_calls("toda_conv3x3_transform_weight_batch", "toda_conv3x3_transform_weight") as calls:
        us = ops.conv3x3_transform_weights_batched(list(zip(ws, modes)))
        assert calls["toda_conv3x3_transform_weight_batch"] == 1 and calls["toda_conv3x3_transform_weight"] == 0
    for w, mode, u in zip(ws, modes, us):
        ref = ops.conv3x3_transform_weight(w, mode)
        assert u.shape == ref.shape and torch.equal(u, ref), (tuple(w.shape), mode)
    # the data-gradient operand alone, and more layers than one launch's table holds (16)
    many = [(ws[i % 3], (0, 1, 2)[i % 3]) for i in range(19)]
    for (w, mode), u in zip(many, ops.conv3x3_transform_weights_batched(many)):
        assert torch.equal(u, ops.conv3x3_transform_weight(w, mode)), (tuple(w.shape), mode)


def test_prepack_caches_on_the_version_counters_and_serves_the_layers():
    from toda_amd import ops

    seq = _stack()
    convs = _convs(seq)
    x = torch.randn(2, 32, 10, 6, device="cuda")
    with H.abi_calls("toda_conv3x3_transform_weight_batch", "toda_conv3x3_transform_weight") as calls:
        assert ops.conv3x3_prepack(list(seq), x) == 3
        assert calls["toda_conv3x3_transform_weight_batch"] == 1
        held = [c.__dict__["_wino_u"] for c in convs]
        assert [e[2] is not None for e in held] == [False, True, True]
        for c, e in zip(convs, held):
            if e[2] is None:
                assert torch.equal(e[1], ops.conv3x3_transform_weight(c.weight.detach(), 0))
            else:
                ref = ops.conv3x3_transform_weight(c.weight.detach(), 2)
                assert torch.equal(e[1], ref[0]) and torch.equal(e[2], ref[1])
        n_single = calls["toda_conv3x3_transform_weight"]
        # unchanged weights: nothing is launched, by the stack or by its layers, and the entries are the same objects
        assert ops.conv3x3_prepack(list(seq), x) == 0
        y = ops.run_dense_sequential(seq, x)
        assert calls["toda_conv3x3_transform_weight_batch"] == 1 and calls["toda_conv3x3_transform_weight"] == n_single
        assert all(c.__dict__["_wino_u"] is e for c, e in zip(convs, held))
        # an in-place update of one layer: that lone layer transforms for itself (the batch is for two and more) ...
        with torch.no_grad():
            convs[1].weight.mul_(0.5)
        assert ops.conv3x3_prepacked(convs[1]) is None and ops.conv3x3_prepack(list(seq), x) == 0
        # ... an update of all of them (and a write through raw pointers, which moves no version counter) rebuilds the batch
        with torch.no_grad():
            for c in convs:
                c.weight.add_(0.01)
        assert ops.conv3x3_prepack(list(seq), x) == 3 and calls["toda_conv3x3_transform_weight_batch"] == 2
        ops.weights_written_in_place()
        assert ops.conv3x3_prepack(list(seq), x) == 3 and calls["toda_conv3x3_transform_weight_batch"] == 3
    for c in convs:
        assert torch.equal(ops.conv3x3_prepacked(c)[0], ops.conv3x3_transform_weight(c.weight.detach(), 0))
    assert y.shape == (2, 32, 10, 6)


def test_stack_through_the_cache_equals_layer_by_layer_forward_and_backward():
    """run_dense_sequential with the batched operands against the same layers each transforming for itself: outputs and every
    gradient bit for bit, also after the two-launch optimizer step has rewritten the weights through raw pointers."""
    from toda_amd import ops
    from toda_amd.tools.train_utils.optimization import OneCycleAdam, clip_and_step

    seq = _stack(3)
    convs = _convs(seq)
    opt = OneCycleAdam(seq, wd=0.01)
    assert opt._hip_step
    x = torch.randn(2, 32, 12, 10, device="cuda")

    def layer_by_layer():
        ws = [c.weight.detach().clone().requires_grad_(True) for c in convs]
        b = convs[2].bias.detach().clone().requires_grad_(True)
        xx = x.clone().requires_grad_(True)
        y = ops.conv3x3(ops.conv3x3(torch.relu(ops.conv3x3(xx, ws[0])), ws[1]), ws[2], b)
        y.square().sum().backward()
        return y.detach(), xx.grad, [w.grad for w in ws]

    for step in range(2):
        xs = x.clone().requires_grad_(True)
        seq.zero_grad()
        with H.abi_calls("toda_conv3x3_transform_weight_batch", "toda_conv3x3_transform_weight") as calls:
            y = ops.run_dense_sequential(seq, xs)
            y.square().sum().backward()
            assert calls["toda_conv3x3_transform_weight_batch"] == 1 and calls["toda_conv3x3_transform_weight"] == 0, step
        y_ref, gx_ref, gw_ref = layer_by_layer()
        assert torch.equal(y.detach(), y_ref) and torch.equal(xs.grad, gx_ref), step
        for c, gw in zip(convs, gw_ref):
            assert torch.equal(c.weight.grad, gw), step
        with H.abi_calls("toda_clip_adam_step") as n:
            clip_and_step(opt, list(seq.parameters()), 10.0)
            assert n["toda_clip_adam_step"] == 1


# (batch, cin, cout, H, W): fewer chunk steps than CUs (a grid below the CU count); partial tiles with several units cut by
# stream-K boundaries; every CU busy with many segments per unit
WGRAD_SHAPES = [(1, 32, 32, 8, 8), (2, 64, 32, 20, 18), (1, 32, 64, 94, 94)]


@pytest.mark.parametrize("shape", WGRAD_SHAPES)
def test_fused_wgrad_fold_equals_the_reduce_finish_pair(shape):
    from toda_amd import ops

    b, cin, cout, h, w_ = shape
    g = torch.Generator().manual_seed(cin * 7 + cout + h)
    x = torch.randn((b, cin, h, w_), generator=g).cuda()
    gy = torch.randn((b, cout, h, w_), generator=g).cuda()
    assert os.environ.get("TODA_WGRAD_FOLD") is None
    dw = ops.conv3x3_wgrad(x, gy, (cout, cin, 3, 3))
    os.environ["TODA_WGRAD_FOLD"] = "pair"
    try:
        ref = ops.conv3x3_wgrad(x, gy, (cout, cin, 3, 3))
    finally:
        del os.environ["TODA_WGRAD_FOLD"]
    assert torch.equal(dw, ref)
    assert torch.equal(dw, ops.conv3x3_wgrad(x, gy, (cout, cin, 3, 3)))           # and reproducible
    # not two copies of one mistake: the gradient itself against float64
    xd, wd = x.double().cpu(), torch.zeros((cout, cin, 3, 3), dtype=torch.float64, requires_grad=True)
    torch.nn.functional.conv2d(xd, wd, padding=1).backward(gy.double().cpu())
    err = float((dw.double().cpu() - wd.grad).abs().max() / wd.grad.abs().max())
    assert err < 5e-5, err
