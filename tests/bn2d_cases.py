"""Case list, routing restatement, float64 references, bound formulas and input builders of the single-pass BatchNorm2d kernels of
toda_amd/csrc/bn2d.hip, shared by test_bn2d_host.py (no GPU) and test_gpu_bn2d_edges.py.  Nothing here imports the library or needs a
device.  The references are float64 numpy written from the definition of training-mode nn.BatchNorm2d (+ ReLU) and its backward
formula; the bounds are derived from the kernels' documented summation scheme (float32 inside a thread, float64 above it) and
from the unit roundoff of float32, none is measured.

Three layers tie every output to the float64 truth:
  1. the saved statistics (and the running ones) against float64 of x alone;
  2. the forward map against float64 arithmetic on x and the SAVED statistics;
  3. the backward against float64 arithmetic on x, dy, the saved statistics and the mask (y_kernel > 0) of the forward.
T is the number of floats one thread accumulates in float32 before float64 takes over: batch * K * V for the per-channel kernels,
K * V for the per-plane ones.  n = batch * hw."""
import numpy as np

U = 2.0 ** -24                         # unit roundoff of float32
EPS = float(np.float32(1e-3))          # the values the C ABI receives (float arguments)
MOMENTUM = float(np.float32(0.01))
BLOCK = 1024
K_OF_V = {4: (1, 2, 3, 4, 8, 9), 1: (4, 9, 18, 36)}
MAX_SYNC_C = 4096
EINVAL = -1

# ---------------------------------------------------------------------------------------------- routing restatement


def pick_k(hwv, v):
    """smallest instantiated K >= vectors per plane and thread (0: none)"""
    need = -(-hwv // BLOCK)
    for k in K_OF_V[v]:
        if k >= need:
            return k
    return 0


def vec_of(hw):
    return 1 if hw & 3 else 4


def floats_per_thread(batch, hw):
    """one workgroup per channel: the register image of 72 floats per thread; 0: unsupported"""
    if batch < 1 or hw < 1:
        return 0
    v = vec_of(hw)
    k = pick_k(hw // v, v)
    if not k or batch not in (1, 2, 4):
        return 0
    return batch * k * v if batch * k * v <= 72 else 0


def split_ok(batch, c, hw):
    """one workgroup per plane: 36 floats of x (and of dy) per thread"""
    if batch not in (2, 4) or c < 1 or c > MAX_SYNC_C or hw < 1:
        return False
    v = vec_of(hw)
    k = pick_k(hw // v, v)
    return k > 0 and k * v <= 36


def supported(batch, c, hw):
    return int(c >= 1 and (floats_per_thread(batch, hw) > 0 or split_ok(batch, c, hw)))


def routes(batch, c, hw, sync, env_split=1):
    """-> {"fwd": route, "bwd": route}; a route is (family, V, K, T) with family "channel" or "split", or None where the entry point
    refuses the shape.  `sync`: a workspace and a non-zero epoch are given."""
    per_channel = floats_per_thread(batch, hw)
    can_split = bool(sync) and split_ok(batch, c, hw)
    if hw < 1 or c < 1:
        return {"fwd": None, "bwd": None}
    v = vec_of(hw)
    k = pick_k(hw // v, v)

    def route(split):
        if split:
            return ("split", v, k, k * v)
        return ("channel", v, k, batch * k * v) if per_channel > 0 else None

    return {"fwd": route(can_split and per_channel == 0),
            "bwd": route(can_split and (per_channel == 0 or (per_channel > 36 and bool(env_split))))}


def instantiation(direction, batch, route):
    """the kernel template instance a route launches: (direction, family, V, batch, K)"""
    family, v, k, _ = route
    return (direction, family, v, batch, k)


def need_of(hw):
    v = vec_of(hw)
    return -(-(hw // v) // BLOCK)


# ---------------------------------------------------------------------------------------------- case list
HW = [1, 3, 4, 5, 4092, 4096, 4100, 4097, 8192, 8196, 12288, 12292, 16384, 16388, 9215, 9217, 18431, 18433, 28672, 32772, 36860,
      36863, 36864]
BATCHES = (1, 2, 4)
SWEEP_C = 3
SWEEP = [(hw, batch) for hw in HW for batch in BATCHES]
# the split routes on the interleaved (C % 8 == 0) and the plain workgroup -> plane mapping
MAPPING_CASES = [(batch, c, hw) for c in (8, 9) for batch, hw in ((4, 16388), (2, 16388), (4, 18433), (4, 8196))]
# V = 1 once more with every tensor one float past a 16-byte boundary
MISALIGNED = [(hw, batch) for hw in HW if vec_of(hw) == 1 for batch in BATCHES]

SPIKE_SHAPES = [(hw, batch) for hw in (4100, 16388, 9217, 36863) for batch in (1, 4)]
NEIGHBOUR_HW = [16388, 4097, 9217, 18433, 5]
SLICE_SHAPES = [(2, 4100), (4, 4097), (4, 9217), (4, 16388), (2, 36863)]
THRESHOLD_SHAPES = [(2, 4100), (1, 8196), (4, 4097), (2, 16388), (4, 9217)]
THRESHOLD_CHANNELS = 8
SPLIT_ONLY = [(4, 16388), (4, 18433)]                      # (batch, hw) that only the per-plane kernels serve
REUSE_SEQUENCE = [(3, 4), (8, 2), (9, 4), (8, 4), (3, 2)]  # (C, P) of consecutive split launches on one workspace
REUSE_EPOCHS = [1, 2, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF]
REUSE_HW = 16388
ENV_SPLIT_SHAPES = [(2, 3, 16388), (4, 3, 9217)]


def spike_positions(hw):
    """flat positions inside a plane around the first and the last k-slice a thread block loads, and the plane's ends"""
    v = vec_of(hw)
    pos = {0, v * BLOCK - 1, v * BLOCK, (need_of(hw) - 1) * v * BLOCK, hw - v, hw - 1}
    return sorted(p for p in pos if 0 <= p < hw)


def reachable(hw_range, batches=BATCHES, c=SWEEP_C):
    """every instantiation the two launchers reach over hw_range x batches x {sync given, NULL}"""
    out = set()
    for hw in hw_range:
        for batch in batches:
            for sync in (True, False):
                r = routes(batch, c, hw, sync)
                for d in ("fwd", "bwd"):
                    if r[d] is not None:
                        out.add(instantiation(d, batch, r[d]))
    return out


# ---------------------------------------------------------------------------------------------- input builders
def _ulp_block(x0, count):
    """count float32 values x0 + i ulp(x0), i cycling through -32 .. 32"""
    x0 = np.float32(x0)
    ulp = float(np.abs(np.spacing(x0)))
    i = (np.arange(count) % 65) - 32
    vals = (float(x0) + i * ulp).astype(np.float32)
    assert np.array_equal(vals.astype(np.float64), float(x0) + i * ulp)       # one binade: exact
    return vals


def zero_crossing(x, gamma, beta):
    """float64 x at which gamma (x - mu) / sqrt(var + eps) + beta changes sign, from the float64 statistics of x"""
    x64 = x.astype(np.float64).ravel()
    mu = x64.mean()
    var = ((x64 - mu) ** 2).mean()
    return mu - float(beta) * np.sqrt(var + EPS) / float(gamma)


THRESHOLD_COUNT = 1025
THRESHOLD_ROUNDS = 60


def threshold_channel(batch, hw, gamma, beta, sign, rng):
    """[batch, hw] float32: mean sign * 1000, sigma 1, and THRESHOLD_COUNT elements (fewer where the channel is small) at random
    positions holding x0 + i ulp, i cycling through -32 .. 32, x0 the float32 nearest the channel's own float64 zero crossing.  The
    block moves the statistics, so x0 is iterated to a fixed point.  -> (x, positions, rounds)"""
    n = batch * hw
    count = min(THRESHOLD_COUNT, n // 4)
    x = (sign * 1000.0 + rng.standard_normal(n)).astype(np.float32)
    if count < 65:
        return x.reshape(batch, hw), np.zeros(0, np.int64), 0
    pos = rng.choice(n, count, replace=False)
    x0 = np.float32(zero_crossing(x, gamma, beta))
    for rounds in range(1, THRESHOLD_ROUNDS + 1):
        x[pos] = _ulp_block(x0, count)
        nxt = np.float32(zero_crossing(x, gamma, beta))
        if nxt == x0:
            return x.reshape(batch, hw), pos, rounds
        x0 = nxt
    raise AssertionError(f"threshold channel did not converge in {THRESHOLD_ROUNDS} rounds (batch {batch}, hw {hw})")


def near_threshold(x_channel, gamma, beta):
    """on the float64 reference alone: (elements with |z| inside the layer 2 bound, how many of them have z > 0)"""
    x64 = x_channel.astype(np.float64).ravel()
    mu = x64.mean()
    var = ((x64 - mu) ** 2).mean()
    s = float(gamma) / np.sqrt(var + EPS)
    z = x64 * s + (float(beta) - mu * s)
    inside = np.abs(z) <= 4 * U * (np.abs(x64 * s) + abs(mu * s) + abs(float(beta)))
    return int(inside.sum()), int((z[inside] > 0).sum())


class Case:
    """Seeded float32 inputs of one (batch, c, hw): channel kinds cycle through well-conditioned N(0.7, 2^2), ill-conditioned mean
    +-1000 / sigma 1 and the threshold channel (plain ill-conditioned data where the channel is too small to hold the block).
    kinds: per channel "w", "i" or "t"; all "t" builds the threshold probe's channels with alternating signs of mean, gamma, beta."""

    def __init__(self, batch, c, hw, seed=None, kinds=None):
        self.batch, self.c, self.hw = batch, c, hw
        rng = np.random.default_rng(1_000_003 * batch + 7919 * c + hw if seed is None else seed)
        kinds = kinds or "".join("wit"[i % 3] for i in range(c))
        assert len(kinds) == c
        self.kinds = kinds
        self.gamma = rng.uniform(0.5, 1.5, c).astype(np.float32)
        self.beta = rng.uniform(0.05, 0.5, c).astype(np.float32) * rng.choice([-1.0, 1.0], c).astype(np.float32)
        if kinds == "t" * c:       # signs of (mean, gamma, beta) run through all eight combinations
            self.gamma *= np.where((np.arange(c) >> 1) & 1, -1, 1).astype(np.float32)
            self.beta = np.abs(self.beta) * np.where((np.arange(c) >> 2) & 1, -1, 1).astype(np.float32)
        self.rm = rng.uniform(-0.3, 0.3, c).astype(np.float32)
        self.rv = rng.uniform(0.5, 2.0, c).astype(np.float32)
        self.x = np.empty((batch, c, hw), np.float32)
        self.threshold_pos, self.threshold_rounds = {}, {}
        for ch, kind in enumerate(kinds):
            sign = -1.0 if ch & 1 else 1.0
            if kind == "w":
                self.x[:, ch] = (0.7 + 2.0 * rng.standard_normal((batch, hw))).astype(np.float32)
            elif kind == "i":
                self.x[:, ch] = (sign * 1000.0 + rng.standard_normal((batch, hw))).astype(np.float32)
            else:
                self.x[:, ch], self.threshold_pos[ch], self.threshold_rounds[ch] = \
                    threshold_channel(batch, hw, self.gamma[ch], self.beta[ch], sign, rng)
        self.dy = rng.standard_normal((batch, c, hw)).astype(np.float32)


def spike_case(batch, hw, plane, pos, c=2, seed=11):
    """x = N(0, 1) and dy = N(0, 1), each with the element `pos` of sample `plane` set to 1000 in every channel"""
    case = Case(batch, c, hw, seed=seed, kinds="w" * c)
    rng = np.random.default_rng(seed + 1)
    case.x = rng.standard_normal((batch, c, hw)).astype(np.float32)
    case.x[plane, :, pos] = 1000.0
    case.dy[plane, :, pos] = 1000.0
    return case


# ---------------------------------------------------------------------------------------------- references and bounds
def stats64(x):
    """float64 (mean, biased variance, mean |x|) per channel of x [batch, c, hw]"""
    x64 = x.astype(np.float64)
    mu = x64.mean((0, 2))
    var = ((x64 - mu[None, :, None]) ** 2).mean((0, 2))
    return mu, var, np.abs(x64).mean((0, 2))


def layer1(x, T, rm0=None, rv0=None):
    """Statistics against float64 of x.  -> dict of name -> (reference, absolute bound), per channel.
    mean: (T - 1) u mean|x| for the float32 partial sums, u |mu| for the final rounding.
    invstd: (T + 2) u on the centred squares, u for the float32 rounding of the variance, u for adding eps, halved by the square root;
    one ulp each for sqrtf and the divide and two more for a device sqrt / divide that is not correctly rounded: (T / 2 + 6) u."""
    mu, var, mabs = stats64(x)
    n = x.shape[0] * x.shape[2]
    mean_b = (T - 1) * U * mabs + U * np.abs(mu)
    inv = 1.0 / np.sqrt(var + EPS)
    out = {"mean": (mu, mean_b), "invstd": (inv, (T / 2 + 6) * U * inv)}
    if rm0 is not None:
        m = MOMENTUM
        unb = var * n / (n - 1) if n > 1 else np.zeros_like(var)
        rm64, rv64 = rm0.astype(np.float64), rv0.astype(np.float64)
        out["running_mean"] = ((1 - m) * rm64 + m * mu, m * mean_b + 3 * U * (np.abs((1 - m) * rm64) + np.abs(m * mu)))
        out["running_var"] = ((1 - m) * rv64 + m * unb, m * (T + 5) * U * unb + 3 * U * (np.abs((1 - m) * rv64) + m * unb))
    return out


def layer2(x, gamma, beta, save, relu):
    """Forward map given the saved statistics: float64 s = gamma invstd, z = x s + (beta - mean s), y = max(z, 0) with ReLU;
    |y - y_ref| <= 4 u (|x s| + |mean s| + |beta|).  -> (z, y_ref, bound), [batch, c, hw]"""
    mean, invstd = save[0].astype(np.float64), save[1].astype(np.float64)
    s = gamma.astype(np.float64) * invstd
    b64 = beta.astype(np.float64)
    x64 = x.astype(np.float64)
    z = x64 * s[None, :, None] + (b64 - mean * s)[None, :, None]
    bound = 4 * U * (np.abs(x64 * s[None, :, None]) + (np.abs(mean * s) + np.abs(b64))[None, :, None])
    return z, (np.maximum(z, 0.0) if relu else z), bound


def layer3(x, dy, gamma, save, mask, T):
    """Backward given the saved statistics and the forward's mask (None: no ReLU).  float64 G = masked dy, xhat = (x - mean) invstd,
    S1 = sum G, S2 = sum G xhat, dx = s (G - S1 / n - xhat S2 / n).  -> dict name -> (reference, bound)."""
    mean, invstd = save[0].astype(np.float64), save[1].astype(np.float64)
    s = gamma.astype(np.float64) * invstd
    n = x.shape[0] * x.shape[2]
    G = dy.astype(np.float64)
    if mask is not None:
        G = np.where(mask, G, 0.0)
    xh = (x.astype(np.float64) - mean[None, :, None]) * invstd[None, :, None]
    S1, S2 = G.sum((0, 2)), (G * xh).sum((0, 2))
    B1 = T * U * np.abs(G).sum((0, 2)) + U * np.abs(S1)
    B2 = (T + 3) * U * np.abs(G * xh).sum((0, 2)) + U * np.abs(S2)
    c = lambda a: a[None, :, None]      # noqa: E731
    dx = c(s) * (G - c(S1 / n) - xh * c(S2 / n))
    dx_b = 6 * U * np.abs(c(s)) * (np.abs(G) + np.abs(c(S1 / n)) + np.abs(xh * c(S2 / n))) + np.abs(c(s)) * (c(B1 / n) + np.abs(xh) * c(B2 / n))
    return {"dbeta": (S1, B1), "dgamma": (S2, B2), "dx": (dx, dx_b)}


def ratio(got, ref, bound):
    """worst |got - ref| / bound; an error of exactly zero counts as 0 even under a zero bound"""
    err = np.abs(np.asarray(got, np.float64) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / bound)
    r = np.where(np.isnan(r), np.inf, r)          # a NaN output misses every bound
    return float(r.max()) if r.size else 0.0


# ---------------------------------------------------------------------------------------------- float32 restatement of the kernels
def _thread_image(plane_list, v, k):
    """[planes * k, 1024, v] float32: the vectors thread t holds, in the order it adds them; zeros past the end of a plane"""
    rows = []
    for p in plane_list:
        buf = np.zeros(k * BLOCK * v, np.float32)
        buf[:p.size] = p
        rows.append(buf.reshape(k, BLOCK, v))
    return np.concatenate(rows)


def _thread_sum(img):
    s = np.zeros(img.shape[1], np.float32)
    for vec in img:
        s = s + (((vec[:, 0] + vec[:, 1]) + (vec[:, 2] + vec[:, 3])) if vec.shape[1] == 4 else vec[:, 0])
    return s


def emulate_forward(xc, gamma, beta, route, relu):
    """One channel xc [batch, hw] through the forward kernels' arithmetic in numpy float32 / float64 (same operation order, no
    contraction).  -> (mean, invstd, y): what a correct kernel gives, up to the device's sqrt and divide."""
    family, v, k, _ = route
    batch, hw = xc.shape
    f32 = np.float32

    def moments(planes):
        img = _thread_image(planes, v, k)
        n = float(sum(p.size for p in planes))
        mean_d = float(_thread_sum(img).astype(np.float64).sum()) / n
        mean = f32(mean_d)
        valid = _thread_image([np.ones(p.size, np.float32) for p in planes], v, k) > 0
        d = np.where(valid, img - mean, f32(0))
        q = np.zeros(BLOCK, np.float32)
        for vec in d:
            for j in range(v):
                q = q + vec[:, j] * vec[:, j]
        dm = mean_d - float(mean)
        return mean_d, float(q.astype(np.float64).sum()) - n * dm * dm, n

    if family == "channel":
        mean_d, m2, n = moments(list(xc))
        var_d = max(m2 / n, 0.0)
    else:
        parts = [moments([p]) for p in xc]
        mean_d = sum(p[0] for p in parts) / batch
        m2 = sum(p[1] + hw * (p[0] - mean_d) ** 2 for p in parts)
        var_d = m2 / (hw * batch) if m2 > 0 else 0.0
    mean = f32(mean_d)
    invstd = f32(1) / np.sqrt(f32(var_d) + f32(EPS))
    scale = f32(gamma) * invstd
    shift = f32(beta) - mean * scale
    z = xc * scale + shift
    return mean, invstd, (np.where(z > 0, z, f32(0)) if relu else z)


def emulate_backward(xc, gc, gamma, beta, mean, invstd, route, relu, mask_expr="forward"):
    """One channel through the backward kernels' arithmetic.  -> (dgamma, dbeta, dx).  mask_expr: "forward" is the kernels' own
    x * scale + shift; "fma" (one rounding) and "centred" ((x - mean) * scale + beta) are the wrong kernels test_bn2d_host.py shows the
    threshold channels to catch."""
    family, v, k, _ = route
    batch, hw = xc.shape
    f32 = np.float32
    mean, invstd = f32(mean), f32(invstd)
    scale = f32(gamma) * invstd
    shift = f32(beta) - mean * scale
    if mask_expr == "forward":
        pre = xc * scale + shift
    elif mask_expr == "fma":           # the product of two float32 is exact in float64
        pre = (xc.astype(np.float64) * float(scale) + float(shift)).astype(np.float32)
    else:
        pre = (xc - mean) * scale + f32(beta)
    g = np.where(pre > 0, gc, f32(0)) if relu else gc
    xh = (xc - mean) * invstd

    def sums(planes_g, planes_t):
        ig, it = _thread_image(planes_g, v, k), _thread_image(planes_t, v, k)
        s1, s2 = np.zeros(BLOCK, np.float32), np.zeros(BLOCK, np.float32)
        for a, b in zip(ig, it):
            for j in range(v):
                s1 = s1 + a[:, j]
                s2 = s2 + b[:, j]
        return float(s1.astype(np.float64).sum()), float(s2.astype(np.float64).sum())

    gx = g * xh
    if family == "channel":
        sum_g, sum_gx = sums(list(g), list(gx))
    else:
        parts = [sums([a], [b]) for a, b in zip(g, gx)]
        sum_g, sum_gx = sum(p[0] for p in parts), sum(p[1] for p in parts)
    n = float(batch * hw)
    m1, m2 = f32(sum_g / n), f32(sum_gx / n)
    dx = scale * (g - m1 - xh * m2)
    return f32(sum_gx), f32(sum_g), dx
