"""What the local-augmentation tests share: the fixture written by tests/golden/capture_local_aug.py (the reference's
outputs, read once and handed out as copies) and the comparison both roads are held to."""
import functools
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "local_aug.npz")
TOL = 2e-5          # rotated / recovered coordinates: a possibly-fused fp32 dot product at <= 16 m plus one rounding at <= 128 m
ROTATED = ("local_rotation",)
SWAPPED = ("local_pyramid_swap", "pyramid_aug")


@functools.lru_cache(maxsize=None)
def _golden():
    with np.load(GOLDEN) as g:
        return {k: g[k] for k in g.files}


def case_names():
    return [str(c) for c in _golden()["cases"]]


def case(name):
    """dict: fn, seed, args (list, ranges as [lo, hi]), points, boxes (fresh copies), out_points, out_boxes, next_draw."""
    g = _golden()
    i = case_names().index(name)
    fn, sk = str(g["fns"][i]), str(g["scenes"][i])
    flat = g[f"{name}.args"].tolist()
    if fn == "pyramid_aug":
        args = [flat[0], flat[1], int(flat[2]), flat[3], int(flat[4])]
    elif fn.startswith("local_pyramid_dropout"):
        args = [flat[0]]
    elif fn.startswith("local_pyramid"):
        args = [flat[0], int(flat[1])]
    elif fn.startswith("random_translation"):
        args = [flat[0]]
    else:
        args = [flat]
    return dict(name=name, fn=fn, seed=int(g[f"{name}.seed"]), args=args, points=g[f"scene.{sk}.points"].copy(), boxes=g[f"scene.{sk}.boxes"].copy(),
                out_points=g[f"{name}.out_points"], out_boxes=g[f"{name}.out_boxes"], next_draw=float(g[f"{name}.next_draw"]))


def membership_calls(name):
    """[(points, pyramids [P, 5, 3], mask bool [n, P])]: what the reference's points_in_pyramids_mask saw in this case."""
    g, c, out = _golden(), case(name), []
    for k in range(int(g[f"{name}.pyr_calls"])):
        if f"{name}.mask{k}.mask" not in g:
            continue
        pts = g.get(f"{name}.mask{k}.points", c["points"])
        pyr = g[f"{name}.mask{k}.pyramids"]
        out.append((pts, pyr, np.unpackbits(g[f"{name}.mask{k}.mask"], axis=0, count=len(pts)).astype(bool)))
    return out


def run(utils, c, boxes, points):
    """Seed, call the function of `utils` the case names (pyramid_aug: the three pyramid functions, pyramids handed on)."""
    np.random.seed(c["seed"])
    if c["fn"] == "pyramid_aug":
        a = c["args"]
        boxes, points, pyr = utils.local_pyramid_dropout(boxes, points, a[0])
        boxes, points, pyr = utils.local_pyramid_sparsify(boxes, points, a[1], a[2], pyr)
        boxes, points = utils.local_pyramid_swap(boxes, points, a[3], a[4], pyr)
    else:
        boxes, points = getattr(utils, c["fn"])(boxes, points, *c["args"])[:2]
    return boxes, points, np.random.uniform()


def _copied_prefix(c):
    """How many leading rows of the reference's output are bit-equal copies of input rows: the rows the swap left alone (with
    what dropout and sparsify kept), which come first.  Taken from the fixture alone."""
    seen = {r.tobytes() for r in c["points"]}
    n = 0
    while n < len(c["out_points"]) and c["out_points"][n].tobytes() in seen:
        n += 1
    return n


def check(c, boxes, points, next_draw):
    """Boxes and the random stream bit-equal; points bit-equal, count and order included.  The tolerance holds only where the
    reference goes through a matmul - x and y of the rows local_rotation turned (those whose x or y the reference changed) -
    or through short dot products - x, y, z of the rows the swap wrote (those after the copied rows).  Returns the largest
    deviation there."""
    points = np.asarray(points)
    want = c["out_points"]
    assert next_draw == c["next_draw"], "np.random was not left where the reference leaves it"
    assert boxes.dtype == c["out_boxes"].dtype and np.array_equal(boxes, c["out_boxes"])
    assert points.shape == want.shape and points.dtype == want.dtype
    loose = np.zeros(want.shape, bool)
    if c["fn"] in ROTATED:
        loose[:, 0:2] = (want[:, 0:2] != c["points"][:, 0:2]).any(1)[:, None]
    elif c["fn"] in SWAPPED:
        loose[_copied_prefix(c):, 0:3] = True
    assert np.array_equal(points[~loose], want[~loose])
    dev = float(np.abs(points[loose].astype(np.float64) - want[loose]).max()) if loose.any() else 0.0
    assert dev <= TOL, dev
    return dev
