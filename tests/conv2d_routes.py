"""The launch decisions of the dense neck kernels restated in plain Python, for tests that must know which kernel, accessor and
work split a shape takes: the pixel-GEMMs of toda_amd/csrc/gemm2d.hip (stride-2 3x3 conv, ConvTranspose2d with k = s in {1, 2})
and the Winograd F(4x4,3x3) convolution of toda_amd/csrc/conv2d.hip.  Every function mirrors one host-side rule of those files;
test_conv2d_routes.py holds the restatement against the library's own size and support queries.

A pixel-GEMM launch (pg_launch) is (r1 rows, r2 columns, gz contraction splits):
  path "split"   pg_kernel<PgSplit> (128 x 128 tiles) for every grid whose contraction is at least one stage
                 (kc >= PG_K); shorter ones take the native kernels
  path "native"  pg_kernel<PgFp32<64>> when gz == 1 and there are fewer than 768 tiles of 128 x 128, else <PgFp32<128>>;
                 the stride-2 data gradient's 4 parity classes in blockIdx.z are counted in the tiles."""

N_CU = 256          # compute units of an MI355X: the stream-K grids below are sized by it

# gemm2d.hip
PG_K = 32           # contraction values per stage
PG_WG_TARGET = 512  # pg_splits: workgroups a weight gradient aims for (TODA_PG_WG_TARGET)
PG_MAX_SPLITS = 512

# conv2d.hip
WN_TILES = 32       # tiles per tile block
WN_COUT = 32        # produced channels per channel block
WN_KC = 8           # contracted channels per chunk
WN_FREQ = 36
WS_MAX_GRID = 256
WG_KT = 8           # tiles per wgrad step
WG_SLAB_FLOATS = WN_FREQ * 32 * 32
WINO_GANG_KB = 2560

# conv2d_narrow.hip
NW_CO = 4
NW_MAX_BRANCH = 8
NW_BAND = 8
NW_MAX_W = 256


def cdiv(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------------------------------------ pixel-GEMMs
def pg_splits(n_pixels, tiles, target=PG_WG_TARGET):
    want = cdiv(target, tiles if tiles > 0 else 1)
    max_by_len = max(n_pixels // (8 * PG_K), 1)
    return max(1, min(want, max_by_len, PG_MAX_SPLITS))


def pg_kernel(path, r1, r2, gz, kc):
    """Kernel of pg_launch for an r1 x r2 result contracting kc values: "split", "native64" or "native128"."""
    if path == "split" and kc >= PG_K:
        return "split"
    return "native64" if gz == 1 and cdiv(r1, 128) * cdiv(r2, 128) < 768 else "native128"


def _wgrad_split(n, splits):
    per = cdiv(cdiv(n, splits), PG_K) * PG_K
    empty = sum(1 for z in range(splits) if z * per >= n)
    return per, empty


def s2_routes(path, b, cin, cout, h, w, target=PG_WG_TARGET):
    """ZeroPad2d(1) + Conv2d(3, stride 2) on [b, cin, h, w]: toda_conv3x3s2_{fwd,dgrad,wgrad}."""
    ho, wo = h // 2, w // 2
    n, k = b * ho * wo, cin * 9
    if path == "split" and cout >= PG_K:          # the one-tap parity class contracts cout values
        dgrad = "split"
    else:
        dgrad = "native64" if cdiv(cin, 128) * cdiv(n, 128) * 4 < 768 else "native128"
    splits = pg_splits(n, cdiv(k, 128) * cdiv(cout, 128), target)
    per, empty = _wgrad_split(n, splits)
    small_map = b * max(cin, cout) * h * w < (1 << 31)
    fast = small_map and (ho * wo) % 4 == 0 and ho * wo >= PG_K and wo >= PG_K
    return {"fwd": pg_kernel(path, cout, n, 1, k), "dgrad": dgrad, "dgrad_classes": 4, "wgrad": pg_kernel(path, cout, k, splits, n),
            "splits": splits, "per": per, "empty": empty, "fast": fast, "pixels": n, "contraction": {"fwd": k, "dgrad": cout * 4}}


def deconv_routes(path, b, cin, cout, h, w, s, target=PG_WG_TARGET):
    """ConvTranspose2d(cin, cout, k = s, stride s) on [b, cin, h, w]: toda_deconv_{fwd,dgrad,wgrad}."""
    n, m = b * h * w, cout * s * s
    splits = pg_splits(n, cdiv(m, 128) * cdiv(cin, 128), target)
    per, empty = _wgrad_split(n, splits)
    small_map = b * max(cin, cout) * h * s * w * s < (1 << 31)
    fast = small_map and (h * w) % 4 == 0 and h * w >= PG_K and (s == 1 or w >= PG_K)
    return {"fwd": pg_kernel(path, m, n, 1, cin), "dgrad": pg_kernel(path, cin, n, 1, m), "wgrad": pg_kernel(path, cin, m, splits, n),
            "splits": splits, "per": per, "empty": empty, "fast": fast, "pixels": n, "contraction": {"fwd": cin, "dgrad": m}}


def s2_wgrad_workspace_bytes(b, cin, cout, h, w, target=PG_WG_TARGET):
    splits = s2_routes("native", b, cin, cout, h, w, target)["splits"]
    return cdiv(splits * cout * cin * 9 * 4, 256) * 256


def deconv_wgrad_workspace_bytes(b, cin, cout, h, w, s, target=PG_WG_TARGET):
    splits = deconv_routes("native", b, cin, cout, h, w, s, target)["splits"]
    return cdiv(splits * cin * cout * s * s * 4, 256) * 256


# ------------------------------------------------------------------------------------------------------------ Winograd
def _max_sharers(G, S, unit_len):
    """Largest number of the G stream-K ranges [w S / G, (w + 1) S / G) that hold steps of one unit of unit_len steps."""
    count = {}
    for r in range(G):
        lo, hi = r * S // G, (r + 1) * S // G
        if hi > lo:
            for u in range(lo // unit_len, (hi - 1) // unit_len + 1):
                count[u] = count.get(u, 0) + 1
    return max(count.values()) if count else 0


def wino_gang(ncb, cin, n_tile_blocks, n_chunks, n_cu=N_CU, gang_kb=WINO_GANG_KB):
    """toda_conv3x3_fwd's gang rule (TODA_WINO_GANG = 1): 0 = no gangs."""
    gang = 0
    if ncb > 1 and ncb <= 32 and 32 % ncb == 0 and n_cu % ncb == 0:
        gang = ncb
        slice_bytes = WN_FREQ * cin * WN_COUT * 4
        while gang > 1 and gang * slice_bytes > gang_kb * 1024:
            gang >>= 1
        if (ncb // gang) * n_tile_blocks * n_chunks < n_cu // gang:
            gang = 0
    return gang


def wino_tiles(b, h, w):
    return b * cdiv(w, 4) * cdiv(h, 4)


def wino_routes(b, cin, cout, h, w, direction="fwd", n_cu=N_CU):
    """Stream-K launch of wino_fwd_ws_kernel for conv2d(x [b, cin, h, w], weight [cout, cin, 3, 3], padding 1); direction "dgrad"
    is the same kernel with the roles swapped (produces cin channels, contracts cout)."""
    ci, co = (cout, cin) if direction == "dgrad" else (cin, cout)
    n_tiles = wino_tiles(b, h, w)
    ntb, ncb, n_chunks = cdiv(n_tiles, WN_TILES), co // WN_COUT, ci // WN_KC
    n_units = ntb * ncb
    gang = wino_gang(ncb, ci, ntb, n_chunks, n_cu)
    steps = n_units * n_chunks
    grid = n_cu if gang else min(steps, n_cu)
    gsz = gang or 1
    ranges = grid // gsz
    seq = ((ncb // gsz) * ntb if gang else n_units) * n_chunks          # steps of the sequence the ranges split
    return {"tiles": n_tiles, "tile_blocks": ntb, "last_block_tiles": n_tiles - (ntb - 1) * WN_TILES, "cout_blocks": ncb,
            "chunks": n_chunks, "units": n_units, "steps": steps, "grid": grid, "gang": gang, "steps_per_wg": seq / ranges,
            "max_wg_per_unit": _max_sharers(ranges, seq, n_chunks)}


def wino_wgrad_routes(b, cin, cout, h, w, n_cu=N_CU):
    """toda_conv3x3_wgrad: units = (32 input x 32 output channel) blocks, steps of WG_KT tiles, stream-K over units x steps."""
    n_tiles = wino_tiles(b, h, w)
    units = (cin // 32) * (cout // 32)
    spu = cdiv(n_tiles, WG_KT)
    steps = units * spu
    grid = min(steps, n_cu)
    return {"tiles": n_tiles, "units": units, "steps_per_unit": spu, "steps": steps, "grid": grid,
            "max_wg_per_unit": _max_sharers(grid, steps, spu)}


def wino_wgrad_workspace_bytes(cin, cout):
    return (WS_MAX_GRID + 2 * (cin // 32) * (cout // 32)) * WG_SLAB_FLOATS * 4


def wino_supported(b, cin, cout, h, w):
    return (b >= 1 and h >= 1 and w >= 2 and w % 2 == 0 and cin >= 32 and cin % 32 == 0 and cout >= 32 and cout % 32 == 0
            and 4 * b * max(cin, cout) * h * w < (1 << 32) - 65536)


# ------------------------------------------------------------------------------------------------------------ narrow convs
def narrow_supported(b, cin, cout, h, w):
    return (b >= 1 and cin >= 1 and 1 <= cout <= NW_CO and h >= 1 and w >= 4 and w % 4 == 0 and w <= NW_MAX_W
            and 4 * b * cin * h * w < (1 << 32) - 65536)


def narrow_bands(b, h):
    return cdiv(b * h, NW_BAND)
