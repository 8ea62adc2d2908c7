"""The consistency term of the stage-2 step (include/toda.h toda_consistency_loss): a numpy oracle of the
definition and the cases the host and the GPU tests share.

A case is a dict of adv [B, Na, cols] fp32, adv_sel [B, Na] uint8, org [B, No, cols] fp32, org_sel [B, No] uint8."""
import numpy as np

F32 = np.float32
MATCH_DIST2 = F32(1.0)
BLOCK = 256                      # rows per tile and per staged chunk of the kernel (consistency.hip CONS_BLOCK)
U = 2.0 ** -24                   # unit roundoff of fp32, round to nearest


def d2_matrix(a, o):
    """[na, no] fp32: ((ax - ox)^2 + (ay - oy)^2) + (az - oz)^2, every operation rounded to fp32, in this order."""
    a, o = np.asarray(a, F32), np.asarray(o, F32)
    with np.errstate(invalid="ignore", over="ignore"):
        dx = a[:, None, 0] - o[None, :, 0]
        dy = a[:, None, 1] - o[None, :, 1]
        dz = a[:, None, 2] - o[None, :, 2]
        d = (dx * dx + dy * dy) + dz * dz
    assert d.dtype == F32
    return d


def nearest(d):
    """(best [n] fp32, partner [n] int, -1 = none) along axis 1.  A NaN is smaller than every number (torch.min's rule): a row
    that meets one has best = NaN and no partner.  No column: best = +inf.  Ties go to the smallest index."""
    n, m = d.shape
    best, part = np.full((n,), np.inf, F32), np.full((n,), -1, np.int64)
    if m == 0:
        return best, part
    nan = np.isnan(d).any(axis=1)
    clean = np.where(np.isnan(d), np.inf, d)
    part = clean.argmin(axis=1)                     # the first of equal minima
    best = clean[np.arange(n), part].astype(F32)
    best[nan], part[nan] = np.nan, -1
    return best, part


def oracle_sample(adv, adv_sel, org, org_sel, match_dist2=MATCH_DIST2):
    """The definition on one sample: partners and `<` decisions from the fp32 distances, sums in float64."""
    adv, org = np.asarray(adv, F32), np.asarray(org, F32)
    ia, io = np.flatnonzero(np.asarray(adv_sel)), np.flatnonzero(np.asarray(org_sel))
    a, o = adv[ia], org[io]
    d = d2_matrix(a[:, :3], o[:, :3])
    best_a, part_a = nearest(d)
    best_o, part_o = nearest(d.T)
    with np.errstate(invalid="ignore"):
        m_a, m_o = best_a < F32(match_dist2), best_o < F32(match_dist2)
    a64, o64 = a.astype(np.float64), o.astype(np.float64)
    centre = np.abs(a64[m_a, :3] - o64[part_a[m_a], :3]).sum() + np.abs(o64[m_o, :3] - a64[part_o[m_o], :3]).sum()
    size = ((a64[m_a, 3:6] - o64[part_a[m_a], 3:6]) ** 2).sum() + ((o64[m_o, 3:6] - a64[part_o[m_o], 3:6]) ** 2).sum()
    return {"centre_sum": float(centre), "size_sum": float(size), "selected": len(ia) + len(io),
            "matched_adv": int(m_a.sum()), "matched_org": int(m_o.sum()), "matched": int(m_a.sum() + m_o.sum()),
            "partner_of_adv": np.where(m_a, io[np.clip(part_a, 0, None)] if len(io) else -1, -1),
            "partner_of_org": np.where(m_o, ia[np.clip(part_o, 0, None)] if len(ia) else -1, -1),
            "best_adv": best_a, "best_org": best_o}


def oracle(case, match_dist2=MATCH_DIST2):
    """(centre, size, per_sample [B, 4] float64 = centre_sum, size_sum, selected, matched, samples = the oracle_sample dicts)."""
    batch = case["adv"].shape[0]
    samples = [oracle_sample(case["adv"][b], case["adv_sel"][b], case["org"][b], case["org_sel"][b], match_dist2) for b in range(batch)]
    per = np.array([[s["centre_sum"], s["size_sum"], s["selected"], s["matched"]] for s in samples], np.float64).reshape(batch, 4)
    n = np.maximum(per[:, 2], 1.0)
    return float((per[:, 0] / n).sum() / batch), float((per[:, 1] / n).sum() / batch), per, samples


def has_both_directions_and_an_unmatched_box(samples):
    return (sum(s["matched_adv"] for s in samples) >= 1 and sum(s["matched_org"] for s in samples) >= 1
            and sum(s["selected"] - s["matched"] for s in samples) >= 1)


# ---- the bound ------------------------------------------------------------------------------------------------------------
def tiles(na, no):
    return max(1, -(-max(na, no) // BLOCK))


def chain_sample(na, no):
    """D for a per-sample sum: the fp32 additions a term passes through in consistency.hip as built.  2 inside the row
    ((t0 + t1) + t2), 6 levels of the width-64 butterfly, 3 across the four waves of the workgroup, 2 * tiles - 1 in cons_fold
    over the (direction, tile) partials of the sample."""
    return 2 + 6 + 3 + 2 * tiles(na, no) - 1


def chain_total(na, no, batch):
    """D for the two results: the per-sample chain and one addition per sample of the batch.  The roundings that are not
    additions (the difference, the square, the division by n, the division by batch) are inside the bound's + 6."""
    return chain_sample(na, no) + batch


def bound(d, value):
    """Every term is non-negative and passes through at most d additions and 4 other roundings, each of relative error at most
    2^-24: |computed - exact| <= ((1 + u)^(d + 4) - 1) * exact <= (d + 6) u * exact for the d of these kernels (d < 100)."""
    return (d + 6) * U * abs(value)


# ---- case builders ---------------------------------------------------------------------------------------------------------
def _lattice(idx, far=0.0):
    """Distinct centres 4 m apart; `far` moves them out of everybody's reach."""
    idx = np.asarray(idx)
    return np.stack([4.0 * (idx % 32) + far, 4.0 * (idx // 32) - 40.0, np.zeros(len(idx))], axis=1)


def random_sample(rng, na, no, cols=7, sel_frac=1.0, poison=False):
    """One sample with partners at a jitter of at most 0.3 m per axis (d2 <= 0.27), some adv boxes that share a partner, and boxes
    out of reach.  adv 0 is the partner pair of org perm[0]; with na >= 2 the last adv box lies out of reach.  `poison`: the
    unselected rows hold inf and NaN."""
    org = rng.uniform(-1, 1, (no, cols))
    org[:, :3] = _lattice(np.arange(no)) + rng.uniform(-0.2, 0.2, (no, 3))
    org[:, 3:6] = rng.uniform(0.5, 5.0, (no, 3))
    adv = rng.uniform(-1, 1, (na, cols))
    adv[:, 3:6] = rng.uniform(0.5, 5.0, (na, 3))
    perm = rng.permutation(no)
    n_pair = max(1, min(na, no) * 6 // 10)
    n_share = min(na - n_pair, n_pair // 3) if na > n_pair + 1 else 0
    for i in range(na):
        if i < n_pair:
            adv[i, :3] = org[perm[i], :3] + rng.uniform(-0.3, 0.3, 3)
        elif i < n_pair + n_share:
            adv[i, :3] = org[perm[i - n_pair], :3] + rng.uniform(-0.3, 0.3, 3)
        else:
            adv[i, :3] = _lattice([i], far=1000.0)[0] + rng.uniform(-0.2, 0.2, 3)
    adv_sel, org_sel = np.ones(na, np.uint8), np.ones(no, np.uint8)
    if sel_frac < 1.0:
        adv_sel, org_sel = (rng.random(na) < sel_frac).astype(np.uint8), (rng.random(no) < sel_frac).astype(np.uint8)
        adv_sel[0], org_sel[perm[0]] = 1, 1
        adv_sel[-1] = 1
        org_sel[perm[-1]] = 1
    adv, org = adv.astype(F32), org.astype(F32)
    if poison:
        for t, s in ((adv, adv_sel), (org, org_sel)):
            off = np.flatnonzero(s == 0)
            t[off[0::2]] = np.inf
            t[off[1::2]] = np.nan
    return adv, adv_sel, org, org_sel


def stack(samples):
    return {"adv": np.stack([s[0] for s in samples]), "adv_sel": np.stack([s[1] for s in samples]),
            "org": np.stack([s[2] for s in samples]), "org_sel": np.stack([s[3] for s in samples])}


def random_case(seed, batch, na, no, cols=7, sel_frac=1.0, poison=False):
    rng = np.random.default_rng(seed)
    return stack([random_sample(rng, na, no, cols, sel_frac, poison) for _ in range(batch)])


def unmatched_single_case(batch=3):
    """(Na, No) = (1, 1): sample 0 and 2 are a pair, sample 1 lies 2 m apart.  A 1 x 1 sample is matched in both directions or in
    none, so only a batch holds a matched pair and an unmatched box together."""
    case = random_case(5, batch, 1, 1)
    case["adv"][1, 0, :3] = case["org"][1, 0, :3] + np.array([2.0, 0.0, 0.0], F32)
    return case


def empty_side_case():
    """Sample 0 as usual, sample 1 with nothing selected in org, sample 2 with nothing selected at all."""
    case = random_case(6, 3, 40, 70, sel_frac=0.7, poison=True)
    case["org_sel"][1] = 0
    case["adv_sel"][2] = 0
    case["org_sel"][2] = 0
    return case


def nan_centre_case():
    """Sample 0: the selected adv row 3 has a NaN x.  Its best is NaN, and so is every org box's (each meets it in its column):
    no org box of the sample is matched, the other adv boxes are.  Sample 1 is clean."""
    case = random_case(7, 2, 30, 45)
    case["adv"][0, 3, 0] = np.nan
    return case


def tie_case(second, swap=False):
    """One box at (10, 10, 0) against 300, two of which - indices 5 and `second` - lie 0.5 m to either side: d2 = 0.25 on both, exactly
    (every coordinate is a multiple of 0.5).  Their sizes differ, so the wrong partner shows in size_sum.  Every other box is out
    of reach.  `swap`: the single box is the org one, so the tie is met by the other direction."""
    n = 300
    many = np.zeros((n, 7), F32)
    many[:, :3] = _lattice(np.arange(n), far=500.0)
    many[:, 3:6] = 2.0
    many[5, :3], many[second, :3] = (10.5, 10.0, 0.0), (9.5, 10.0, 0.0)
    many[5, 3:6], many[second, 3:6] = (1.0, 1.5, 2.0), (3.0, 3.5, 4.0)
    one = np.zeros((1, 7), F32)
    one[0, :3], one[0, 3:6] = (10.0, 10.0, 0.0), (1.5, 1.5, 1.5)
    adv, org = (many, one) if swap else (one, many)
    return stack([(adv, np.ones(len(adv), np.uint8), org, np.ones(len(org), np.uint8))])


def _threshold_offset():
    """fp32 (dx, dy) with ((dx^2 + dy^2) + 0) == nextafter(1, 0) in fp32 arithmetic, found by search."""
    target = np.nextafter(F32(1.0), F32(0.0))
    for k in range(1, 16):
        dy = F32(k / 16.0)
        x0 = F32(np.sqrt(np.float64(target) - np.float64(dy) ** 2))
        x = x0
        for _ in range(64):
            x = np.nextafter(x, F32(0.0))
        for _ in range(128):
            if F32(F32(x * x) + F32(dy * dy)) == target:
                return x, dy
            x = np.nextafter(x, F32(2.0))
    raise AssertionError("no fp32 offset with d2 == nextafter(1, 0)")


def threshold_case():
    """Sample 0: d2 exactly 1.0 (dx = 1): unmatched.  Sample 1: d2 = nextafter(1, 0): matched.  A second adv box out of reach in
    both."""
    dx, dy = _threshold_offset()
    samples = []
    for off in ((F32(1.0), F32(0.0)), (dx, dy)):
        org = np.zeros((1, 7), F32)
        org[0, 3:6] = (1.0, 2.0, 3.0)
        adv = np.zeros((2, 7), F32)
        adv[0, :3], adv[0, 3:6] = (off[0], off[1], 0.0), (1.5, 2.5, 3.5)
        adv[1, :3], adv[1, 3:6] = (500.0, 0.0, 0.0), (1.0, 1.0, 1.0)
        samples.append((adv, np.ones(2, np.uint8), org, np.ones(1, np.uint8)))
    return stack(samples)


SHAPES = [(1, 1), (257, 1), (1, 300), (255, 515), (24, 24)]


def parity_cases():
    """{name: case}: everything the kernel is compared with the oracle on."""
    cases = {}
    for na, no in SHAPES:
        for batch in (1, 3):
            if (na, no) == (1, 1) and batch == 3:
                cases["1x1_b3"] = unmatched_single_case(3)
            else:
                cases[f"{na}x{no}_b{batch}"] = random_case(100 + na + no + batch, batch, na, no)
    cases["empty_sides"] = empty_side_case()
    cases["poisoned_unselected"] = random_case(8, 2, 300, 280, sel_frac=0.4, poison=True)
    cases["nan_centre"] = nan_centre_case()
    cases["tie_5_261"] = tie_case(261)
    cases["tie_5_6"] = tie_case(6)
    cases["tie_5_261_swapped"] = tie_case(261, swap=True)
    cases["tie_5_6_swapped"] = tie_case(6, swap=True)
    cases["threshold"] = threshold_case()
    cases["cols7"] = random_case(9, 2, 50, 60, cols=7)
    cases["cols9"] = random_case(10, 2, 50, 60, cols=9, sel_frac=0.6)
    return cases


def as_lists(case, padded):
    """The per-sample lists get_consistency_loss takes, as numpy: padded (every row, with `mask`) or unpadded (the selected rows)."""
    adv, org = [], []
    for b in range(case["adv"].shape[0]):
        sa, so = case["adv_sel"][b].astype(bool), case["org_sel"][b].astype(bool)
        if padded:
            adv.append({"pred_boxes": case["adv"][b].copy(), "mask": sa})
            org.append({"pred_boxes": case["org"][b].copy(), "mask": so})
        else:
            adv.append({"pred_boxes": case["adv"][b][sa].copy()})
            org.append({"pred_boxes": case["org"][b][so].copy()})
    return adv, org
