"""toda_consistency_loss (consistency.hip) against the numpy oracle of the definition at the kernel's edges, and
get_consistency_loss on device lists against the torch composition."""
import numpy as np
import pytest
import torch

from tests import consistency_cases as C
from toda_amd import lib as L
from toda_amd import ops
from toda_amd.pcdet import models as M

pytestmark = pytest.mark.gpu

CASES = C.parity_cases()
ORACLE = {name: C.oracle(case) for name, case in CASES.items()}           # computed once, shared, never written to


def run(case):
    dev = torch.device("cuda:0")
    t = {k: torch.from_numpy(v).to(dev) for k, v in case.items()}
    centre, size, per = ops.consistency_match(t["adv"], t["adv_sel"], t["org"], t["org_sel"])
    return np.float32(centre.item()), np.float32(size.item()), per.cpu().numpy()


def check_against_oracle(name, got, where=""):
    case = CASES[name]
    centre, size, per, samples = ORACLE[name]
    batch, na, no = case["adv"].shape[0], case["adv"].shape[1], case["org"].shape[1]
    g_centre, g_size, g_per = got
    print(f"{name}{where}: centre {g_centre!r} vs {centre!r}, size {g_size!r} vs {size!r}")
    np.testing.assert_array_equal(g_per[:, 3], per[:, 3], err_msg=f"{name}: matched counts")
    np.testing.assert_array_equal(g_per[:, 2], per[:, 2], err_msg=f"{name}: selected counts")
    d_s, d_t = C.chain_sample(na, no), C.chain_total(na, no, batch)
    for b in range(batch):
        for col, what in ((0, "centre_sum"), (1, "size_sum")):
            err, lim = abs(float(g_per[b, col]) - per[b, col]), C.bound(d_s, per[b, col])
            print(f"  sample {b} {what}: {g_per[b, col]!r} vs {per[b, col]!r}, error {err:.3e}, bound {lim:.3e}")
            assert err <= lim, (name, b, what, err, lim)
    for value, ref, what in ((g_centre, centre, "centre"), (g_size, size, "size")):
        err, lim = abs(float(value) - ref), C.bound(d_t, ref)
        assert err <= lim, (name, what, err, lim)


@pytest.mark.parametrize("name", sorted(CASES))
def test_kernel_equals_the_oracle_and_repeats_its_bits(name):
    _, _, per, samples = ORACLE[name]
    if name != "1x1_b1":      # a single 1 x 1 sample is matched in both directions or in none: no room for an unmatched box
        assert C.has_both_directions_and_an_unmatched_box(samples)
    else:
        assert samples[0]["matched_adv"] == 1 and samples[0]["matched_org"] == 1
    first = run(CASES[name])
    check_against_oracle(name, first)
    second = run(CASES[name])
    assert first[0].tobytes() == second[0].tobytes() and first[1].tobytes() == second[1].tobytes()
    assert first[2].tobytes() == second[2].tobytes()


def test_bool_selection_and_views_of_the_results():
    case = CASES["255x515_b3"]
    dev = torch.device("cuda:0")
    t = {k: torch.from_numpy(v).to(dev) for k, v in case.items()}
    a = ops.consistency_match(t["adv"], t["adv_sel"], t["org"], t["org_sel"])
    b = ops.consistency_match(t["adv"], t["adv_sel"].bool(), t["org"], t["org_sel"].bool())
    assert a[0].dim() == 0 and a[2].shape == (3, 4) and not a[0].requires_grad
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])


def test_bad_arguments_return_an_error_with_a_message():
    lib = L.load()
    dev = torch.device("cuda:0")
    boxes = torch.zeros((1, 4, 7), device=dev)
    sel = torch.ones((1, 4), dtype=torch.uint8, device=dev)
    out = torch.zeros((6,), device=dev)
    need = lib.toda_consistency_workspace_bytes(1, 4, 4)
    assert need >= 2 * 16
    ws = torch.zeros((need,), dtype=torch.uint8, device=dev)
    p = L.ptr

    def call(na=4, no=4, batch=1, cols=7, ws_bytes=need, adv=boxes, out_=out):
        return lib.toda_consistency_loss(p(adv), p(sel), na, p(boxes), p(sel), no, batch, cols, 1.0, p(out_), p(ws), ws_bytes, L.stream())

    assert call() == 0
    assert call(batch=0) != 0 and b"batch" in lib.toda_last_error()
    assert call(na=-1) != 0 and b"na >= 0" in lib.toda_last_error()
    assert call(cols=5) != 0 and b"6 columns" in lib.toda_last_error()
    assert call(ws_bytes=need - 1) != 0 and b"workspace" in lib.toda_last_error()
    assert call(adv=None) != 0 and b"null adv" in lib.toda_last_error()
    assert call(out_=None) != 0 and b"null out" in lib.toda_last_error()
    with pytest.raises(RuntimeError, match="float32"):
        ops.consistency_match(boxes.double(), sel, boxes.double(), sel)
    with pytest.raises(RuntimeError, match="adv_sel"):
        ops.consistency_match(boxes, sel[:, :3], boxes, sel)
    torch.cuda.synchronize()


def device_lists(lists):
    return [{k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in d.items()} for d in lists]


@pytest.mark.parametrize("name,padded", [("255x515_b3", True), ("cols9", True), ("poisoned_unselected", True),
                                         ("255x515_b3", False), ("cols9", False), ("poisoned_unselected", False), ("empty_sides", False)])
def test_get_consistency_loss_on_device_lists_equals_the_torch_composition(name, padded):
    """Padded lists with masks (CenterPoint) and unpadded lists of unequal lengths (SECOND-IoU)."""
    case = CASES[name]
    adv, org = C.as_lists(case, padded)
    if not padded and name != "255x515_b3":
        assert len({len(d["pred_boxes"]) for d in adv}) > 1 or len({len(d["pred_boxes"]) for d in org}) > 1        # unequal lengths
    got = M.get_consistency_loss(device_lists(adv), device_lists(org))
    ref = M._consistency_loss_torch(device_lists(adv), device_lists(org))
    batch, na, no = case["adv"].shape[0], case["adv"].shape[1], case["org"].shape[1]
    d_t = C.chain_total(na, no, batch)
    for g, r, what in zip(got, ref, ("centre", "size")):
        assert torch.is_tensor(g) and g.is_cuda
        g, r = float(g), float(r)
        print(f"{name} padded={padded} {what}: kernel route {g!r}, torch composition {r!r}, bound {C.bound(d_t, r):.3e}")
        assert abs(g - r) <= C.bound(d_t, r), (name, what, g, r)
    check_against_oracle(name, (np.float32(float(got[0])), np.float32(float(got[1])), ORACLE[name][2].astype(np.float32)), where=" (lists)")


def test_get_consistency_loss_adds_no_synchronisation():
    case = CASES["cols7"]
    for padded in (True, False):
        adv, org = C.as_lists(case, padded)
        adv, org = device_lists(adv), device_lists(org)
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            M.get_consistency_loss(adv, org)
        finally:
            torch.cuda.set_sync_debug_mode("default")
