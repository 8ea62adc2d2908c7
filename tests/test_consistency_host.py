"""The numpy oracle of the consistency term (tests/consistency_cases.py) against the reference fixture, the CPU torch forms of
get_consistency_loss and the definition's edge rules.  No GPU."""
import os

import numpy as np
import pytest
import torch

from tests import consistency_cases as C
from toda_amd.pcdet import models as M

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def torch_lists(lists):
    return [{k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in d.items()} for d in lists]


def test_oracle_reproduces_the_reference_fixture():
    z = np.load(os.path.join(G, "consistency.npz"))
    centre = size = 0.0
    for i in range(3):
        a, o = z[f"adv{i}"], z[f"org{i}"]
        s = C.oracle_sample(a, np.ones(len(a), np.uint8), o, np.ones(len(o), np.uint8))
        n = max(1, s["selected"])
        centre, size = centre + s["centre_sum"] / n, size + s["size_sum"] / n
    np.testing.assert_allclose(centre / 3, float(z["center_loss"]), rtol=1e-6)
    np.testing.assert_allclose(size / 3, float(z["size_loss"]), rtol=1e-6)
    assert float(z["center_loss"]) > 0 and float(z["size_loss"]) > 0


@pytest.mark.parametrize("padded", [True, False])
@pytest.mark.parametrize("seed,batch,na,no,frac", [(1, 1, 24, 24, 1.0), (2, 3, 255, 515, 1.0), (3, 2, 60, 33, 0.5), (4, 4, 1, 300, 1.0)])
def test_oracle_agrees_with_the_cpu_torch_forms(padded, seed, batch, na, no, frac):
    case = C.random_case(seed, batch, na, no, sel_frac=frac)
    centre, size, per, samples = C.oracle(case)
    assert C.has_both_directions_and_an_unmatched_box(samples)
    adv, org = C.as_lists(case, padded)
    got_c, got_s = M.get_consistency_loss(torch_lists(adv), torch_lists(org))
    # the torch forms sum in fp32 in an order of their own: a loose bound here, the kernel's own is in test_gpu_consistency.py
    np.testing.assert_allclose(float(got_c), centre, rtol=2e-5)
    np.testing.assert_allclose(float(got_s), size, rtol=2e-5)
    again = M._consistency_loss_torch(torch_lists(adv), torch_lists(org))
    assert float(again[0]) == float(got_c) and float(again[1]) == float(got_s)           # host tensors take the torch forms


def test_every_parity_case_matches_in_both_directions_and_leaves_a_box_unmatched():
    for name, case in C.parity_cases().items():
        _, _, _, samples = C.oracle(case)
        if name == "1x1_b1":
            # a single 1 x 1 sample is matched in both directions or in none: it cannot hold an unmatched box as well
            assert samples[0]["matched_adv"] == 1 and samples[0]["matched_org"] == 1
            continue
        assert C.has_both_directions_and_an_unmatched_box(samples), name


def test_nan_distance_is_smaller_than_every_number():
    case = C.nan_centre_case()
    _, _, per, samples = C.oracle(case)
    s = samples[0]
    assert np.isnan(s["best_adv"][3]) and s["partner_of_adv"][3] == -1
    assert np.isnan(s["best_org"]).all() and s["matched_org"] == 0          # every org box meets the NaN row
    assert s["matched_adv"] >= 1 and np.isfinite(per).all()
    assert samples[1]["matched_org"] >= 1
    # torch.min's rule, which the definition copies
    v, i = torch.tensor([[3.0, float("nan"), 0.5, float("nan")]]).min(1)
    assert torch.isnan(v).all() and int(i) == 1


@pytest.mark.parametrize("second", [6, 261])
@pytest.mark.parametrize("swap", [False, True])
def test_a_tie_goes_to_the_smaller_index(second, swap):
    case = C.tie_case(second, swap)
    _, _, per, samples = C.oracle(case)
    s = samples[0]
    one, many = ("org", "adv") if swap else ("adv", "org")
    assert s[f"best_{one}"][0] == np.float32(0.25) and s[f"partner_of_{one}"][0] == 5
    assert s[f"matched_{one}"] == 1 and s[f"matched_{many}"] == 2 and s["selected"] == 301
    d5 = np.array([1.5, 1.5, 1.5]) - np.array([1.0, 1.5, 2.0])
    d2nd = np.array([1.5, 1.5, 1.5]) - np.array([3.0, 3.5, 4.0])
    assert per[0, 1] == pytest.approx(2 * (d5 ** 2).sum() + (d2nd ** 2).sum(), rel=1e-12)      # 5 twice (both directions), `second` once
    assert per[0, 0] == pytest.approx(1.5, rel=1e-12)


def test_the_threshold_is_strict():
    case = C.threshold_case()
    _, _, per, samples = C.oracle(case)
    assert samples[0]["best_adv"][0] == np.float32(1.0) and samples[0]["matched"] == 0 and per[0, 0] == 0.0
    assert samples[1]["best_adv"][0] == np.nextafter(np.float32(1.0), np.float32(0.0)) and samples[1]["matched"] == 2
    assert per[1, 2] == 3 and per[1, 1] == pytest.approx(2 * 0.75)


def test_empty_sides_contribute_nothing_and_still_count_in_the_batch():
    case = C.empty_side_case()
    centre, size, per, samples = C.oracle(case)
    assert samples[1]["matched"] == 0 and np.isinf(samples[1]["best_adv"]).all() and samples[1]["selected"] > 0
    assert samples[2]["selected"] == 0 and samples[2]["matched"] == 0
    assert centre == pytest.approx(per[0, 0] / per[0, 2] / 3) and size == pytest.approx(per[0, 1] / per[0, 2] / 3)
    # the unpadded CPU form skips such samples and divides by the batch as well
    adv, org = C.as_lists(case, padded=False)
    got_c, got_s = M.get_consistency_loss(torch_lists(adv), torch_lists(org))
    np.testing.assert_allclose([float(got_c), float(got_s)], [centre, size], rtol=2e-5)


def test_the_bench_tool_fails_without_a_gpu(monkeypatch):
    from toda_amd.tools import bench_consistency
    monkeypatch.setattr("sys.argv", ["bench_consistency", "--out", ""])
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(SystemExit, match="needs a GPU"):
        bench_consistency.main()
