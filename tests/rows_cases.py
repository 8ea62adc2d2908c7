"""References and case tables of the row passes and scatters of toda_amd/csrc/dense.hip, shared by test_rows_host.py (no GPU) and
test_gpu_rows_edges.py.  Every reference is float64 numpy written from the definition of the operation (nn.BatchNorm1d's
bookkeeping, the BatchNorm backward formula, a gather), none is derived from a kernel; test_rows_host.py checks them against
torch's float64 autograd."""
import math

import numpy as np

from oracle import oracle as O

EPS = float(np.float32(1e-3))          # the values the C ABI receives (float arguments)
MOMENTUM = float(np.float32(0.01))
U24 = 2.0 ** -24                       # unit roundoff of float32

# ---------------------------------------------------------------------------------------------- documented launch plans
MOM_ROWS, MOM_MAX_BLOCKS, EW_BLOCK, EW_MAX_BLOCKS = 256, 2048, 256, 2048


def reduce_plan(n):
    """(blocks, rows_per_block) of the row reductions: 256 rows per block while that gives <= 2048 blocks."""
    n = max(n, 1)
    blocks = min(MOM_MAX_BLOCKS, -(-n // MOM_ROWS))
    return blocks, -(-n // blocks)


def reduce_doubles(n, c):
    return 2 * c * (1 + reduce_plan(n)[0])


def ew_blocks(n, c):
    """Blocks of the elementwise passes: <= 2048 of 256 float4 each, rounded up until a block row holds whole rows of c."""
    g = max(1, min(EW_MAX_BLOCKS, -(-(max(n, 0) * c // 4) // EW_BLOCK)))
    while (g * 1024) % c:
        g += 1
    return g


def colsum_doubles(n, c):
    """Doubles of the column-sum workspace: one slot per channel and elementwise block; a single double when there are no rows."""
    return c * ew_blocks(n, c) if n > 0 else 1


def thread_terms(n, c):
    """T: the most float32 terms one thread of a row reduction adds (everything above a thread is float64)."""
    return -(-reduce_plan(n)[1] // (1024 // c))


# ---------------------------------------------------------------------------------------------- case tables
ROW_C = [4, 8, 16, 32, 64, 128]


def row_counts(c):
    rp = 1024 // c
    return sorted({1, 2, rp - 1, rp, rp + 1, 2 * rp - 1, 2 * rp, 2 * rp + 1, 3 * rp + 1, 255, 256, 257, 511, 513} - {0})


# above 2048 blocks of 256 rows (first two) / above 2048 x 256 float4 of the elementwise grid (first and third)
CAPPED = [(524289, 4), (524288 + 300, 8), (16385, 128)]
ROW_CASES = [(n, c) for c in ROW_C for n in row_counts(c)]
AFFINE_C = [4, 12, 20, 96, 100, 384, 1000, 1024]
AFFINE_CASES = [(n, c) for c in AFFINE_C for n in (1, 3, 257, 2048 * 256 * 4 // c + 1)]
SMALL = 2 ** 16                        # n * c up to here: every element is compared, test_rows_host.py vouches for the seeds
MEAN_SHIFT = (0.0, 0.25)               # stats with the batch mean / with mean + 0.25 * (j + 1) / c, as the column-sum test does

# Seeds: 1000 * c + n, moved on by 7919 * SEED_BUMP[...] where the first draw puts a pre-activation within 1e-4 of zero.
SEED_BUMP = {
    # (n, c, residual, shifted): k, from find_bump below; test_rows_host.py asserts the property for every entry of the table
    (257, 4, True, True): 1, (512, 4, False, False): 1, (512, 4, False, True): 2, (256, 8, True, True): 1,
    (511, 8, False, False): 2, (511, 8, True, False): 1, (513, 8, True, True): 1, (63, 16, True, False): 1,
    (64, 16, False, False): 1, (64, 16, True, True): 1, (128, 16, True, False): 1, (129, 16, True, True): 1,
    (255, 16, True, False): 1, (256, 16, False, False): 2, (256, 16, False, True): 1, (256, 16, True, False): 1,
    (257, 16, False, False): 1, (257, 16, True, False): 1, (511, 16, False, False): 1, (511, 16, True, False): 2,
    (511, 16, True, True): 3, (513, 16, False, True): 1, (33, 32, False, True): 1, (97, 32, False, True): 1,
    (97, 32, True, False): 1, (255, 32, False, True): 5, (256, 32, False, True): 7, (256, 32, True, False): 2,
    (257, 32, True, False): 1, (511, 32, True, False): 3, (513, 32, False, True): 2, (513, 32, True, False): 2,
    (33, 64, False, False): 1, (33, 64, False, True): 1, (49, 64, True, False): 1, (255, 64, False, False): 4,
    (255, 64, False, True): 2, (256, 64, False, False): 4, (256, 64, True, True): 1, (257, 64, True, True): 6,
    (511, 64, False, False): 21, (511, 64, False, True): 30, (511, 64, True, False): 2, (511, 64, True, True): 14,
    (513, 64, False, False): 12, (513, 64, False, True): 65, (513, 64, True, True): 6, (16, 128, False, True): 1,
    (16, 128, True, True): 1, (17, 128, False, True): 1, (17, 128, True, True): 1, (255, 128, False, False): 1,
    (255, 128, False, True): 4, (255, 128, True, False): 6, (255, 128, True, True): 2, (256, 128, False, False): 7,
    (256, 128, False, True): 1, (256, 128, True, False): 2, (256, 128, True, True): 9, (257, 128, False, False): 27,
    (257, 128, False, True): 9, (257, 128, True, True): 1, (511, 128, False, False): 128, (511, 128, False, True): 67,
    (511, 128, True, False): 30, (511, 128, True, True): 11,
}


def seed_of(n, c, residual, shifted):
    return 1000 * c + n + 7919 * SEED_BUMP.get((n, c, bool(residual), bool(shifted)), 0)


class Case:
    """Inputs of one BatchNorm row case: x = randn * 1.3 + 0.1, dy = randn + 0.5 x, the shortcut, gamma, beta and the float32
    stats [mean | invstd | scale | shift] computed in float64 from x and cast."""

    def __init__(self, n, c, residual, shifted, seed=None):
        rng = np.random.default_rng(seed_of(n, c, residual, shifted) if seed is None else seed)
        self.n, self.c = n, c
        self.x = (rng.standard_normal((n, c)) * 1.3 + 0.1).astype(np.float32)
        self.dy = (rng.standard_normal((n, c)).astype(np.float32) + np.float32(0.5) * self.x).astype(np.float32)
        self.res = rng.standard_normal((n, c)).astype(np.float32) if residual else None
        self.gamma = rng.uniform(0.5, 1.5, c).astype(np.float32)
        self.beta = rng.uniform(-0.5, 0.5, c).astype(np.float32)
        x64 = self.x.astype(np.float64)
        mean = x64.mean(0) + (MEAN_SHIFT[1] if shifted else 0.0) * np.arange(1, c + 1) / c
        invstd = 1.0 / np.sqrt(x64.var(0) + EPS)
        scale = self.gamma.astype(np.float64) * invstd
        self.stats = np.stack([mean, invstd, scale, self.beta.astype(np.float64) - mean * scale]).astype(np.float32)

    def pre64(self):
        p = self.x.astype(np.float64) * self.stats[2].astype(np.float64) + self.stats[3].astype(np.float64)
        return p + self.res.astype(np.float64) if self.res is not None else p

    def pre32(self):
        return pre_fp32(self.x, self.stats[2], self.stats[3], self.res)


def find_bump(n, c, residual, shifted, limit=2000):
    """Smallest k whose seed keeps every |pre| above 1e-4 (how SEED_BUMP was filled)."""
    for k in range(limit):
        case = Case(n, c, residual, shifted, seed=1000 * c + n + 7919 * k)
        if np.abs(case.pre64()).min() > 1e-4:
            return k
    raise RuntimeError((n, c, residual, shifted))


# ---------------------------------------------------------------------------------------------- references
def moments(x):
    """(sum x, sum fp32(x*x), sum |x|, sum x^2) per column, all taken in float64."""
    x = np.asarray(x, np.float32)
    x64 = x.astype(np.float64)
    return x64.sum(0), (x * x).astype(np.float64).sum(0), np.abs(x64).sum(0), (x64 * x64).sum(0)


def pre_fp32(x, scale, shift, res=None):
    """The pre-activation in float32 with the kernels' operation order: x * scale, + shift, + res - one rounding each."""
    p = np.asarray(x, np.float32) * np.asarray(scale, np.float32)
    p = p + np.asarray(shift, np.float32)
    if res is not None:
        p = p + np.asarray(res, np.float32)
    assert p.dtype == np.float32
    return p


def affine_act(x, scale, shift, res, relu):
    p = pre_fp32(x, scale, shift, res)
    return np.where(p > 0, p, np.float32(0)) if relu else p


def finalize(sums, n, gamma, beta, rm, rv, momentum, eps, training):
    """nn.BatchNorm1d's bookkeeping in float64 -> (mean, invstd, scale, shift, running_mean', running_var').  Biased variance,
    clamped at 0, for the normalisation; unbiased (n / (n - 1); the biased value for n == 1) into the running estimate."""
    sums = np.asarray(sums, np.float64)
    c = sums.shape[0] // 2
    rm = None if rm is None else np.asarray(rm, np.float64)
    rv = None if rv is None else np.asarray(rv, np.float64)
    if training:
        mean = sums[:c] / n
        var = np.maximum(sums[c:] / n - mean * mean, 0.0)
        if rm is not None:
            unbiased = var * n / (n - 1) if n > 1 else var
            rm, rv = (1 - momentum) * rm + momentum * mean, (1 - momentum) * rv + momentum * unbiased
    else:
        mean, var = rm, rv
    invstd = 1.0 / np.sqrt(var + eps)
    g = np.ones(c) if gamma is None else np.asarray(gamma, np.float64)
    b = np.zeros(c) if beta is None else np.asarray(beta, np.float64)
    return mean, invstd, g * invstd, b - mean * g * invstd, rm, rv


def bn_bwd(dy, x, res, stats32, gamma, relu, mask=None):
    """(dz, dbeta, dgamma, dx) in float64 from the float32 stats the kernel gets: dz = dy * mask, dbeta = sum dz,
    dgamma = sum dz xhat, dx = gamma invstd (dz - dbeta / n - xhat dgamma / n) - also for a mean that is not the batch mean.
    mask: the ReLU mask to use in place of the float64 one, for tensors so large that a few pre-activations lie within float32
    rounding of zero, where both masks are right."""
    dy, x = np.asarray(dy, np.float64), np.asarray(x, np.float64)
    mean, invstd, scale, shift = (np.asarray(s, np.float64) for s in stats32)
    n = x.shape[0]
    dz = dy
    if relu:
        pre = x * scale + shift
        if res is not None:
            pre = pre + np.asarray(res, np.float64)
        dz = dy * ((pre > 0) if mask is None else mask)
    xhat = (x - mean) * invstd
    dbeta, dgamma = dz.sum(0), (dz * xhat).sum(0)
    dx = np.asarray(gamma, np.float64) * invstd * (dz - dbeta / n - xhat * dgamma / n)
    return dz, dbeta, dgamma, dx


def fold_order(p):
    """Sum over the last axis of p [..., blocks] in float64 in the documented fixed order of the folds: thread t adds p[t],
    p[t + 256], ... in turn, then a halving tree over the 256 threads.  Adding the +0.0 of an idle thread is exact."""
    p = np.asarray(p, np.float64)
    k = -(-p.shape[-1] // 256)
    pad = np.zeros(p.shape[:-1] + (k * 256,))
    pad[..., :p.shape[-1]] = p
    pad = pad.reshape(p.shape[:-1] + (k, 256))
    acc = np.zeros(p.shape[:-1] + (256,))
    for i in range(k):
        acc = acc + pad[..., i, :]
    w = 128
    while w:
        acc = acc[..., :w] + acc[..., w:2 * w]
        w //= 2
    return acc[..., 0]


def exact_sum(p):
    """Correctly rounded sum over the last axis."""
    p = np.asarray(p, np.float64)
    return np.array([math.fsum(r) for r in p.reshape(-1, p.shape[-1])]).reshape(p.shape[:-1])


# ---------------------------------------------------------------------------------------------- scatters
SCATTER_N = [0, 1, 63, 64, 65, 129]
SCATTER_C = [1, 5, 31, 32, 33, 65]
SCATTER_BATCH = [1, 3]
DENSE_SHAPE = [2, 5, 7]
PILLAR_NY, PILLAR_NX = 5, 7


def scatter_case(n, c, batch, shape, seed):
    """(idx [n, 4] int32 (b, z, y, x) in shuffled order, feat [n, c]).  The rows hold cell (0, 0, 0) of sample 0 and the last
    cell of the last sample (n == 1: the last cell).  [2, 5, 7] x 3 samples has 210 cells and the 5 x 7 canvas 105, fewer than
    some n of the table: rows past the cell count revisit cells, and every row of a cell carries the same features, so that the
    scatter's result does not depend on which of them is written last; the gather is defined either way."""
    rng = np.random.default_rng(seed)
    vol = int(np.prod(shape))
    cells = batch * vol
    if n == 0:
        lin = np.zeros((0,), np.int64)
    elif n == 1:
        lin = np.array([cells - 1])
    else:
        inner = rng.permutation(np.arange(1, cells - 1))[:max(0, min(n, cells) - 2)]
        lin = np.concatenate([[0, cells - 1], inner])
        if n > len(lin):
            lin = np.concatenate([lin, rng.integers(0, cells, n - len(lin))])
        lin = lin[rng.permutation(n)]
    b, sp = np.divmod(lin, vol)
    z, rem = np.divmod(sp, shape[1] * shape[2])
    y, x = np.divmod(rem, shape[2])
    idx = np.stack([b, z, y, x], 1).astype(np.int32).reshape(n, 4)
    table = rng.standard_normal((cells, c)).astype(np.float32)
    return idx, table[lin].reshape(n, c)


def dense_fwd(feat, idx, batch, shape):
    return O.sparse_to_dense_fwd(feat, idx, batch, shape)


def dense_bwd(gdense, idx, shape):
    return O.sparse_to_dense_bwd(gdense, idx, shape)


def pillar_fwd(feat, idx, batch, ny, nx):
    return O.pillar_scatter_fwd(feat, idx, batch, ny, nx)


def pillar_bwd(gcanvas, idx):
    """The gather of the canvas gradient: cell z + y * nx + x of sample b, every channel."""
    g = np.asarray(gcanvas, np.float32)
    nx = g.shape[3]
    flat = g.reshape(g.shape[0], g.shape[1], -1)
    idx = np.asarray(idx, np.int64).reshape(-1, 4)
    return flat[idx[:, 0], :, idx[:, 1] + idx[:, 2] * nx + idx[:, 3]]
