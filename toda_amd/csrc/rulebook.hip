// Grid index (bitmap + popcount rank) and rulebook (neighbour table) builders for gfx950.
//
// spconv builds its indice pairs with a GPU hash table; on MI355X the lattice of one sparse level
// fits comfortably in HBM as a bitmap (Waymo stride-1 level, batch 2: 185 M cells = 23 MB incl.
// prefix words), so membership + row id become one 8-byte load: cell = {32 occupancy bits,
// popcount of all earlier cells}; rank = cell.y + popc(cell.x & below).  Ranks enumerate sites in
// ascending ((b*D+z)*H+y)*W+x order, which is the canonical row order of every generated set, so
// strided-conv outputs need no sort and no hash probing.  Pure 4/8-byte index traffic: HBM / L2
// latency bound.
#include "grid_index.cuh"
#include "scan.cuh"

namespace toda {

constexpr int RB_BLOCK = GI_TILE;

__global__ void __launch_bounds__(RB_BLOCK)
gi_mark_coords_kernel(const int4* __restrict__ idx, int n, const int32_t* __restrict__ n_dev, GridDims g,
                      uint2* __restrict__ cells) {
    n = eff_n(n, n_dev);
    const int i = blockIdx.x * RB_BLOCK + threadIdx.x;
    if (i >= n) return;
    const int4 c = idx[i];  // (b, z, y, x)
    if (!in_grid(c, g)) return;
    gi_set_bit_first(cells, lin_index(c.x, c.y, c.z, c.w, g));      // (no pre-test; who came first is not asked)
}

__global__ void __launch_bounds__(RB_BLOCK)
gi_rowof_kernel(const int4* __restrict__ idx, int n, const int32_t* __restrict__ n_dev, GridDims g,
                const uint2* __restrict__ cells, int* __restrict__ rowof) {
    n = eff_n(n, n_dev);
    const int i = blockIdx.x * RB_BLOCK + threadIdx.x;
    if (i >= n) return;
    const int4 c = idx[i];
    if (!in_grid(c, g)) return;
    const int r = gi_rank(cells, lin_index(c.x, c.y, c.z, c.w, g));
    rowof[r] = i;
}

struct ConvGeom {
    int ks[3], st[3], pd[3];
    GridDims out;
};

// output coordinate reached from input coordinate `i` through tap `k`, or -1
__device__ __forceinline__ int out_coord(int i, int k, int s, int p, int out_dim) {
    int t = i + p - k;
    if (t < 0) return -1;
    if (s != 1) {
        if (t % s) return -1;
        t /= s;
    }
    return t < out_dim ? t : -1;
}

// input coordinate behind tap `k` of output coordinate `o` (may lie off the lattice)
__device__ __forceinline__ int in_coord(int o, int k, int s, int p) { return o * s - p + k; }

// coordinate of tap `k` of `kn` around a submanifold site
__device__ __forceinline__ int subm_coord(int c, int k, int kn, int d) { return c + (k - kn / 2) * d; }

__global__ void __launch_bounds__(RB_BLOCK)
gi_mark_conv_kernel(const int4* __restrict__ idx, int n, const int32_t* __restrict__ n_dev, ConvGeom cg,
                    uint2* __restrict__ cells) {
    n = eff_n(n, n_dev);
    const int i = blockIdx.x * RB_BLOCK + threadIdx.x;
    if (i >= n) return;
    const int4 c = idx[i];
    if ((unsigned)c.x >= (unsigned)cg.out.B) return;      // the spatial axes are clamped by out_coord
    for (int kz = 0; kz < cg.ks[0]; ++kz) {
        const int zo = out_coord(c.y, kz, cg.st[0], cg.pd[0], cg.out.D);
        if (zo < 0) continue;
        for (int ky = 0; ky < cg.ks[1]; ++ky) {
            const int yo = out_coord(c.z, ky, cg.st[1], cg.pd[1], cg.out.H);
            if (yo < 0) continue;
            for (int kx = 0; kx < cg.ks[2]; ++kx) {
                const int xo = out_coord(c.w, kx, cg.st[2], cg.pd[2], cg.out.W);
                if (xo < 0) continue;
                gi_set_bit(cells, lin_index(c.x, zo, yo, xo, cg.out));
            }
        }
    }
}

// one thread per cell: write the coordinates of its set bits at their ranks
__global__ void __launch_bounds__(RB_BLOCK)
gi_decode_kernel(const uint2* __restrict__ cells, long long n_cells, GridDims g, int4* __restrict__ idx_out, int cap,
                 const int32_t* __restrict__ total_dev, int32_t* __restrict__ n_out_dev) {
    const long long w = (long long)blockIdx.x * RB_BLOCK + threadIdx.x;
    if (w == 0 && n_out_dev) *n_out_dev = *total_dev;
    if (w >= n_cells) return;
    const uint2 c = cells[w];
    unsigned bits = c.x;
    int r = (int)c.y;
    while (bits) {
        const int t = __ffs(bits) - 1;
        bits &= bits - 1;
        if (r < cap) idx_out[r] = lin_coords((w << 5) + t, g, n_cells);
        ++r;
    }
}

// ---- round 4: O(sites) index of an UNORDERED coordinate list (the voxel level) ------------------------------------------
// The voxel level is the big lattice (Waymo, batch 2: 185 M cells = 46 MB of {bits, prefix} words for 0.3 M sites) and its
// rows are in voxel order anyway (rowof maps rank -> row), so its ranks need not be canonical: instead of a popcount scan
// over every word, the site that set the LOWEST bit of a word allocates popc(word) consecutive ranks for it from a counter
// (one atomic per wave).  mark -> alloc -> rowof touch only the occupied words; gi_clear puts them back to zero afterwards,
// so neither a memset nor a scan ever sweeps the lattice.  cell.y = first rank of the word, exactly what gi_rank reads.
__global__ void __launch_bounds__(RB_BLOCK)
gi_mark_first_kernel(const int4* __restrict__ idx, int n, const int32_t* __restrict__ n_dev, GridDims g,
                     uint2* __restrict__ cells, unsigned char* __restrict__ rowmask, int* __restrict__ first,
                     int32_t* __restrict__ counter) {
    n = eff_n(n, n_dev);
    const int i = blockIdx.x * RB_BLOCK + threadIdx.x;
    if (i == 0) *counter = 0;
    if (i >= n) return;
    const int4 c = idx[i];
    int mine = 0;
    if (in_grid(c, g)) {
        mine = gi_set_bit_first(cells, lin_index(c.x, c.y, c.z, c.w, g));      // exactly one of several rows with the same coordinate
        rowmask[row_index(c.x, c.y, c.z, g)] = 1;                               // plain store: every writer stores the same value
    }
    first[i] = mine;
}

constexpr int GA_BLOCK = 1024;
__global__ void __launch_bounds__(GA_BLOCK)
gi_alloc_kernel(const int4* __restrict__ idx, int n, const int32_t* __restrict__ n_dev, GridDims g, uint2* __restrict__ cells,
                const int* __restrict__ first, int32_t* __restrict__ counter) {
    __shared__ int s_base;
    n = eff_n(n, n_dev);
    const int i = blockIdx.x * GA_BLOCK + threadIdx.x;
    int want = 0;
    long long w = 0;
    if (i < n && first[i]) {
        const int4 c = idx[i];
        const long long lin = lin_index(c.x, c.y, c.z, c.w, g);
        w = lin >> 5;
        const unsigned bits = cells[w].x, bit = 1u << (lin & 31);
        if (!(bits & (bit - 1))) want = __popc(bits);       // this row set the word's lowest bit: it allocates for the word
    }
    // ONE atomic per 1024 rows: adds to one address serialise at ~12 ns each at the memory side (one per wave: 58-120 us for a
    // 300 k-row level, measured; one per block: ~4 us)
    int total;
    const int before = block_exclusive_scan<GA_BLOCK>(want, &total);
    if (threadIdx.x == 0) s_base = total ? atomicAdd(counter, total) : 0;
    __syncthreads();
    if (want) cells[w].y = (unsigned)(s_base + before);
}

// un-mark: the words of the listed sites back to {0, 0} (plain stores; rows sharing a word store the same value)
__global__ void __launch_bounds__(RB_BLOCK)
gi_clear_kernel(const int4* __restrict__ idx, int n, const int32_t* __restrict__ n_dev, GridDims g, uint2* __restrict__ cells,
                unsigned char* __restrict__ rowmask) {
    n = eff_n(n, n_dev);
    const int i = blockIdx.x * RB_BLOCK + threadIdx.x;
    if (i >= n) return;
    const int4 c = idx[i];
    if (!in_grid(c, g)) return;
    cells[lin_index(c.x, c.y, c.z, c.w, g) >> 5] = make_uint2(0u, 0u);
    rowmask[row_index(c.x, c.y, c.z, g)] = 0;
}

// ---- round 4: output set of a strided convolution from the input BITMAP, no atomics ---------------------------------------
// gi_mark_conv_kernel sets up to prod(ceil(k / s)) output bits per input site with device atomics (1 M for the voxel level
// of a Waymo batch; they execute at the memory side at ~20 G/s: 55 us per level on average, the most expensive index kernel
// of round 3).  Output-stationary instead: one thread per output WORD ORs the input rows (kz, ky) that reach it - read as
// unaligned bit windows of the input bitmap - and compacts the x axis with the stride.  Every word of the output bitmap is
// written (zero or not): it needs no clearing, and the block's popcount goes straight to the scan's partial sums.
__device__ __forceinline__ unsigned bits32_at(const uint2* __restrict__ cells, long long p, long long lo, long long hi) {
    // 32 bitmap bits starting at linear position p (any alignment); positions outside [lo, hi) read as zero
    const long long a = p > lo ? p : lo, e = (p + 32) < hi ? (p + 32) : hi;
    if (a >= e) return 0u;
    const long long w0 = a >> 5;
    const unsigned lo_word = cells[w0].x;
    const unsigned hi_word = ((e - 1) >> 5) > w0 ? cells[w0 + 1].x : 0u;
    const unsigned long long v = (((unsigned long long)hi_word << 32) | lo_word) >> (a & 31);
    const unsigned cnt = (unsigned)(e - a);
    const unsigned m = cnt >= 32u ? ~0u : ((1u << cnt) - 1u);
    return ((unsigned)v & m) << (unsigned)(a - p);
}

constexpr int CONV_WIN = 4;      // 32-bit windows per input row segment: (count - 1) * sx + KX <= 128 bits

__global__ void __launch_bounds__(RB_BLOCK)
gi_conv_bits_kernel(const uint2* __restrict__ cells_in, const unsigned char* __restrict__ rowmask_in, GridDims gin, ConvGeom cg,
                    uint2* __restrict__ cells_out, long long n_cells_out, int32_t* __restrict__ partials) {
    const long long w = (long long)blockIdx.x * RB_BLOCK + threadIdx.x;
    const GridDims go = cg.out;
    const long long total_bits = (long long)go.B * go.D * go.H * go.W;
    unsigned word = 0u;
    if (w < n_cells_out) {
        long long pos = w << 5;
        const long long end = (pos + 32) < total_bits ? (pos + 32) : total_bits;
        while (pos < end) {
            // the run of this word inside one output row (b, zo, yo)
            const int4 o = lin_coords(pos, go, n_cells_out);      // (b, zo, yo, xo)
            const int room = go.W - o.w;
            const int count = (int)((end - pos) < room ? (end - pos) : room);
            const int xi0 = in_coord(o.w, 0, cg.st[2], cg.pd[2]);
            unsigned win[CONV_WIN] = {0u, 0u, 0u, 0u};
            const int nwin = ((count - 1) * cg.st[2] + cg.ks[2] + 31) >> 5;
            for (int kz = 0; kz < cg.ks[0]; ++kz) {
                const int zi = in_coord(o.y, kz, cg.st[0], cg.pd[0]);
                if ((unsigned)zi >= (unsigned)gin.D) continue;
                for (int ky = 0; ky < cg.ks[1]; ++ky) {
                    const int yi = in_coord(o.z, ky, cg.st[1], cg.pd[1]);
                    if ((unsigned)yi >= (unsigned)gin.H) continue;
                    const long long rix = row_index(o.x, zi, yi, gin);
                    if (rowmask_in && !rowmask_in[rix]) continue;       // an input row without a site (one byte instead of up to 8 words)
                    const long long row = rix * gin.W;
#pragma unroll
                    for (int q = 0; q < CONV_WIN; ++q)
                        if (q < nwin) win[q] |= bits32_at(cells_in, row + xi0 + 32 * q, row, row + gin.W);
                }
            }
            // output bit j = OR over kx of window bit j * sx + kx
            unsigned seg = 0u;
            const unsigned long long lo64 = ((unsigned long long)win[1] << 32) | win[0], hi64 = ((unsigned long long)win[3] << 32) | win[2];
            if ((lo64 | hi64) && cg.st[2] <= 2 && cg.ks[2] <= 8) {
                // stride 1 / 2 (every layer of the reference's backbones): shift-OR over the taps, then keep every stride-th bit
                unsigned long long u = 0ull;
                for (int kx = 0; kx < cg.ks[2]; ++kx) u |= kx ? ((lo64 >> kx) | (hi64 << (64 - kx))) : lo64;
                if (cg.st[2] == 2) {
                    u &= 0x5555555555555555ull;
                    u = (u | (u >> 1)) & 0x3333333333333333ull;
                    u = (u | (u >> 2)) & 0x0f0f0f0f0f0f0f0full;
                    u = (u | (u >> 4)) & 0x00ff00ff00ff00ffull;
                    u = (u | (u >> 8)) & 0x0000ffff0000ffffull;
                    u = (u | (u >> 16)) & 0x00000000ffffffffull;
                }
                seg = (unsigned)u & (count >= 32 ? ~0u : ((1u << count) - 1u));
            } else if (lo64 | hi64) {
                for (int j = 0; j < count; ++j) {
                    unsigned hit = 0u;
                    for (int kx = 0; kx < cg.ks[2]; ++kx) {
                        const int bp = j * cg.st[2] + kx;
                        hit |= (win[bp >> 5] >> (bp & 31)) & 1u;
                    }
                    seg |= hit << j;
                }
            }
            word |= seg << (unsigned)(pos - (w << 5));
            pos += count;
        }
        cells_out[w] = make_uint2(word, 0u);
    }
    int tot;
    block_exclusive_scan(__popc(word), &tot);
    if (threadIdx.x == 0) partials[blockIdx.x] = tot;
}

// ranks of a bitmap whose per-256-word popcounts are in `partials`: every block sums the partials before it, scans its own
// words, stores the prefix words and decodes its sites in canonical order; the last thread publishes the total
__global__ void __launch_bounds__(RB_BLOCK)
gi_scan_decode_kernel(uint2* __restrict__ cells, long long n_cells, const int32_t* __restrict__ partials, GridDims g,
                      int4* __restrict__ idx_out, int cap, int32_t* __restrict__ total_dev, int32_t* __restrict__ n_out_dev) {
    int s = 0;
    for (int k = threadIdx.x; k < (int)blockIdx.x; k += RB_BLOCK) s += partials[k];
    int before;
    block_exclusive_scan(s, &before);
    const long long w = (long long)blockIdx.x * RB_BLOCK + threadIdx.x;
    unsigned bits = w < n_cells ? cells[w].x : 0u;
    int tot;
    int r = before + block_exclusive_scan(__popc(bits), &tot);
    if (w < n_cells) cells[w].y = (unsigned)r;
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == RB_BLOCK - 1) {
        const int all = r + __popc(bits);
        *total_dev = all;
        if (n_out_dev) *n_out_dev = all;
    }
    if (bits) {
        // coordinates of the word's first cell once (32-bit arithmetic when the lattice allows), then carries per set bit
        const int4 first = lin_coords(w << 5, g, n_cells);
        int b = first.x, z = first.y, y = first.z, x = first.w;
        int at = 0;
        while (bits) {
            const int t = __ffs(bits) - 1;
            bits &= bits - 1;
            x += t - at;
            at = t;
            while (x >= g.W) {          // the word runs over the end of a row (W < 32 or no multiple of 32)
                x -= g.W;
                if (++y == g.H) {
                    y = 0;
                    if (++z == g.D) {
                        z = 0;
                        ++b;
                    }
                }
            }
            if (r < cap) idx_out[r] = make_int4(b, z, y, x);
            ++r;
        }
    }
}

// per-block per-offset pair counters: wave ballots -> LDS -> one global atomic per block and offset
__device__ __forceinline__ void pairs_open(int* s_cnt, int k_n) {
    if (threadIdx.x < k_n) s_cnt[threadIdx.x] = 0;
    __syncthreads();
}

__device__ __forceinline__ void count_pairs(bool valid, int k, int* s_cnt) {
    const unsigned long long vote = __ballot(valid);
    if ((threadIdx.x & 63) == 0 && vote) atomicAdd(&s_cnt[k], __popcll(vote));
}

__device__ __forceinline__ void pairs_flush(const int* s_cnt, int k_n, int* __restrict__ pair_cnt) {
    __syncthreads();
    if (threadIdx.x < k_n && s_cnt[threadIdx.x]) atomicAdd(&pair_cnt[threadIdx.x], s_cnt[threadIdx.x]);
}

// tap (kz, ky, kx) of table row k = (kz * KY + ky) * KX + kx
struct Tap {
    int z, y, x;
};
template <int KY, int KX>
__device__ __forceinline__ Tap tap_of(int k) {
    return Tap{k / (KY * KX), (k / KX) % KY, k % KX};
}
// SubM rulebook, one thread per output site.  The K lookups of a site are independent, so they
// are issued as K back-to-back 8-byte cell loads (then K rowof loads) before anything is consumed:
// one round trip to L2/MALL per phase instead of one per offset.  k-major table => the stores of
// a wave are 256 contiguous bytes per offset.
template <int KZ, int KY, int KX>
__global__ void __launch_bounds__(RB_BLOCK)
rb_subm_kernel(const int4* __restrict__ idx, int n, GridDims g, int dz, int dy, int dx,
               const uint2* __restrict__ cells, const int* __restrict__ rowof, int* __restrict__ nbr,
               int* __restrict__ pair_cnt) {
    constexpr int K = KZ * KY * KX;
    __shared__ int s_cnt[K];
    pairs_open(s_cnt, K);
    const int o = blockIdx.x * RB_BLOCK + threadIdx.x;
    const bool live = o < n;
    int4 c = make_int4(0, 0, 0, 0);
    if (live) c = idx[o];
    const bool inside = live && in_grid(c, g);
    uint2 cell[K];
    unsigned bit[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const Tap t = tap_of<KY, KX>(k);
        const int z = subm_coord(c.y, t.z, KZ, dz), y = subm_coord(c.z, t.y, KY, dy), x = subm_coord(c.w, t.x, KX, dx);
        // (a named flag, as this loop always had: with the test written into the `if` the 3x3x3 allocation drops below the
        // 96-register line and the occupancy moves from 4 to 5 waves, which nobody has timed)
        const bool ok = inside && in_lattice(z, y, x, g);
        cell[k] = make_uint2(0u, 0u);
        bit[k] = 0u;
        if (ok) gi_fetch(cells, lin_index(c.x, z, y, x, g), cell[k], bit[k]);
    }
    int r[K];
#pragma unroll
    for (int k = 0; k < K; ++k) r[k] = gi_rank_of(cell[k], bit[k]);
    if (rowof) {
#pragma unroll
        for (int k = 0; k < K; ++k)
            if (r[k] >= 0) r[k] = rowof[r[k]];
    }
#pragma unroll
    for (int k = 0; k < K; ++k) {
        if (live) nbr[(size_t)k * n + o] = r[k];
        count_pairs(r[k] >= 0, k, s_cnt);
    }
    pairs_flush(s_cnt, K, pair_cnt);
}

// generic kernel sizes (K <= 64): same structure, runtime loops
__global__ void __launch_bounds__(RB_BLOCK)
rb_subm_generic_kernel(const int4* __restrict__ idx, int n, GridDims g, int kz_n, int ky_n, int kx_n, int dz, int dy,
                       int dx, const uint2* __restrict__ cells, const int* __restrict__ rowof, int* __restrict__ nbr,
                       int* __restrict__ pair_cnt) {
    __shared__ int s_cnt[64];
    pairs_open(s_cnt, 64);
    const int o = blockIdx.x * RB_BLOCK + threadIdx.x;
    const bool live = o < n;
    int4 c = make_int4(0, 0, 0, 0);
    if (live) c = idx[o];
    const bool inside = live && in_grid(c, g);
    int k = 0;
    for (int kz = 0; kz < kz_n; ++kz)
        for (int ky = 0; ky < ky_n; ++ky)
            for (int kx = 0; kx < kx_n; ++kx, ++k) {
                const int z = subm_coord(c.y, kz, kz_n, dz), y = subm_coord(c.z, ky, ky_n, dy), x = subm_coord(c.w, kx, kx_n, dx);
                uint2 cell = {};
                unsigned bit = 0u;
                if (inside && in_lattice(z, y, x, g)) gi_fetch(cells, lin_index(c.x, z, y, x, g), cell, bit);
                int r = gi_rank_of(cell, bit);
                if (r >= 0 && rowof) r = rowof[r];
                if (live) nbr[(size_t)k * n + o] = r;
                count_pairs(r >= 0, k, s_cnt);
            }
    pairs_flush(s_cnt, k, pair_cnt);
}

// strided conv rulebook, one thread per input site; same issue-all-loads-first structure.
// o2i == nullptr: only the input -> output table and the pair counts (the output -> input table then comes from
// rb_conv_o2i_kernel, output stationary, with complete coalesced stores instead of a 0xFF fill + scattered 4-byte stores)
template <int KZ, int KY, int KX>
__global__ void __launch_bounds__(RB_BLOCK)
rb_conv_kernel(const int4* __restrict__ idx, int n_in, ConvGeom cg, const uint2* __restrict__ cells, int n_out,
               int* __restrict__ o2i, int* __restrict__ i2o, int* __restrict__ pair_cnt) {
    constexpr int K = KZ * KY * KX;
    __shared__ int s_cnt[K];
    pairs_open(s_cnt, K);
    const int i = blockIdx.x * RB_BLOCK + threadIdx.x;
    const bool live = i < n_in;
    int4 c = make_int4(0, 0, 0, 0);
    if (live) c = idx[i];
    const bool inside = live && (unsigned)c.x < (unsigned)cg.out.B;      // the spatial axes are clamped by out_coord
    int zo[KZ], yo[KY], xo[KX];
#pragma unroll
    for (int a = 0; a < KZ; ++a) zo[a] = out_coord(c.y, a, cg.st[0], cg.pd[0], cg.out.D);
#pragma unroll
    for (int a = 0; a < KY; ++a) yo[a] = out_coord(c.z, a, cg.st[1], cg.pd[1], cg.out.H);
#pragma unroll
    for (int a = 0; a < KX; ++a) xo[a] = out_coord(c.w, a, cg.st[2], cg.pd[2], cg.out.W);
    uint2 cell[K];
    unsigned bit[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const Tap t = tap_of<KY, KX>(k);
        cell[k] = make_uint2(0u, 0u);
        bit[k] = 0u;
        if (inside && zo[t.z] >= 0 && yo[t.y] >= 0 && xo[t.x] >= 0) gi_fetch(cells, lin_index(c.x, zo[t.z], yo[t.y], xo[t.x], cg.out), cell[k], bit[k]);
    }
#pragma unroll
    for (int k = 0; k < K; ++k) {
        int o = gi_rank_of(cell[k], bit[k]);
        if (o >= n_out) o = -1;
        if (o >= 0 && o2i) o2i[(size_t)k * n_out + o] = i;
        if (live) i2o[(size_t)k * n_in + i] = o;
        count_pairs(o >= 0, k, s_cnt);
    }
    pairs_flush(s_cnt, K, pair_cnt);
}

// output -> input table of a strided convolution, one thread per OUTPUT site: the input coordinate behind tap k is
// o * stride - pad + k; its row comes from the INPUT level's grid index (rank, then rowof for the voxel level).
template <int KZ, int KY, int KX>
__global__ void __launch_bounds__(RB_BLOCK)
rb_conv_o2i_kernel(const int4* __restrict__ idx_out, int n_out, ConvGeom cg, GridDims gin, const uint2* __restrict__ cells_in,
                   const int* __restrict__ rowof_in, int n_in, int* __restrict__ o2i) {
    constexpr int K = KZ * KY * KX;
    const int o = blockIdx.x * RB_BLOCK + threadIdx.x;
    if (o >= n_out) return;
    const int4 c = idx_out[o];
    uint2 cell[K];
    unsigned bit[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const Tap t = tap_of<KY, KX>(k);
        cell[k] = make_uint2(0u, 0u);
        bit[k] = 0u;
        const int z = in_coord(c.y, t.z, cg.st[0], cg.pd[0]), y = in_coord(c.z, t.y, cg.st[1], cg.pd[1]), x = in_coord(c.w, t.x, cg.st[2], cg.pd[2]);
        if (in_grid(make_int4(c.x, z, y, x), gin)) gi_fetch(cells_in, lin_index(c.x, z, y, x, gin), cell[k], bit[k]);
    }
    int r[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
        r[k] = gi_rank_of(cell[k], bit[k]);
        if (r[k] >= n_in) r[k] = -1;
    }
    if (rowof_in) {
#pragma unroll
        for (int k = 0; k < K; ++k)
            if (r[k] >= 0) r[k] = rowof_in[r[k]];
    }
#pragma unroll
    for (int k = 0; k < K; ++k) o2i[(size_t)k * n_out + o] = r[k];
}

__global__ void __launch_bounds__(RB_BLOCK)
rb_conv_generic_kernel(const int4* __restrict__ idx, int n_in, ConvGeom cg, const uint2* __restrict__ cells, int n_out,
                       int* __restrict__ o2i, int* __restrict__ i2o, int* __restrict__ pair_cnt) {
    __shared__ int s_cnt[64];
    pairs_open(s_cnt, 64);
    const int i = blockIdx.x * RB_BLOCK + threadIdx.x;
    const bool live = i < n_in;
    int4 c = make_int4(0, 0, 0, 0);
    if (live) c = idx[i];
    const bool inside = live && (unsigned)c.x < (unsigned)cg.out.B;
    int k = 0;
    for (int kz = 0; kz < cg.ks[0]; ++kz) {
        const int zo = out_coord(c.y, kz, cg.st[0], cg.pd[0], cg.out.D);
        for (int ky = 0; ky < cg.ks[1]; ++ky) {
            const int yo = out_coord(c.z, ky, cg.st[1], cg.pd[1], cg.out.H);
            for (int kx = 0; kx < cg.ks[2]; ++kx, ++k) {
                const int xo = out_coord(c.w, kx, cg.st[2], cg.pd[2], cg.out.W);
                uint2 cell = {};
                unsigned bit = 0u;
                if (inside && zo >= 0 && yo >= 0 && xo >= 0) gi_fetch(cells, lin_index(c.x, zo, yo, xo, cg.out), cell, bit);
                int o = gi_rank_of(cell, bit);
                if (o >= n_out) o = -1;
                if (o >= 0) o2i[(size_t)k * n_out + o] = i;
                if (live) i2o[(size_t)k * n_in + i] = o;
                count_pairs(o >= 0, k, s_cnt);
            }
        }
    }
    pairs_flush(s_cnt, k, pair_cnt);
}

// the table kernels of one kernel size: the 3x3x3 and 3x1x1 layers of the backbones have unrolled ones, and only those have an
// output-stationary o2i kernel
struct ConvKernels {
    decltype(&rb_conv_generic_kernel) i2o;
    decltype(&rb_conv_o2i_kernel<3, 3, 3>) o2i;
};

static ConvKernels conv_kernels(const int32_t* ks) {
    if (ks[0] == 3 && ks[1] == 3 && ks[2] == 3) return {rb_conv_kernel<3, 3, 3>, rb_conv_o2i_kernel<3, 3, 3>};
    if (ks[0] == 3 && ks[1] == 1 && ks[2] == 1) return {rb_conv_kernel<3, 1, 1>, rb_conv_o2i_kernel<3, 1, 1>};
    return {rb_conv_generic_kernel, nullptr};
}

// the common opening of the strided entry points: the output lattice and its buffer, then the geometry against both shapes
static int conv_setup(const char* who, int batch, const int32_t* shape_in, const int32_t* ks, const int32_t* st, const int32_t* pd,
                      const int32_t* shape_out, const void* gi_out, GiView* out, ConvGeom* cg) {
    int rc = gi_view(who, gi_out, batch, shape_out, out);
    if (rc) return rc;
    for (int a = 0; a < 3; ++a) {
        TODA_CHECK_ARG(ks[a] >= 1 && st[a] >= 1 && pd[a] >= 0, "%s: bad kernel/stride/pad on axis %d", who, a);
        // (C division rounds towards zero: without this an axis one short of its kernel would pass as one output cell)
        TODA_CHECK_ARG(shape_in[a] + 2 * pd[a] >= ks[a], "%s: axis %d of %d cells (+ 2 * %d) is shorter than the kernel's %d", who, a,
                       shape_in[a], pd[a], ks[a]);
        const int expect = (shape_in[a] + 2 * pd[a] - ks[a]) / st[a] + 1;
        TODA_CHECK_ARG(shape_out[a] == expect, "%s: shape_out[%d]=%d but (in+2p-k)/s+1=%d", who, a, shape_out[a], expect);
        cg->ks[a] = ks[a];
        cg->st[a] = st[a];
        cg->pd[a] = pd[a];
    }
    TODA_CHECK_ARG(ks[0] * ks[1] * ks[2] <= 64, "%s: kernel volume > 64 unsupported", who);
    cg->out = out->dims;
    return TODA_OK;
}

}  // namespace toda

using namespace toda;

extern "C" size_t toda_gridindex_bytes(int batch, const int32_t* shape_host) {
    return gi_layout(batch, shape_host).bytes;
}

extern "C" int toda_gridindex_from_coords(const int32_t* idx, int n, const int32_t* n_dev, int batch,
                                          const int32_t* shape_host, void* gi, int32_t* rowof, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    GiView v;
    int rc = gi_view("gridindex_from_coords", gi, batch, shape_host, &v);
    if (rc) return rc;
    TODA_CHECK_ARG(n >= 0, "gridindex_from_coords: n < 0");
    TODA_HIP(hipMemsetAsync(v.cells, 0, (size_t)v.n_cells * sizeof(uint2), s));
    const dim3 grid(cdiv(n, RB_BLOCK)), block(RB_BLOCK);
    if (n > 0) hipLaunchKernelGGL(gi_mark_coords_kernel, grid, block, 0, s, (const int4*)idx, n, n_dev, v.dims, v.cells);
    rc = exclusive_scan(CellAccess{v.cells}, v.n_cells, v.part, v.total, s);
    if (rc) return rc;
    if (n > 0 && rowof)
        hipLaunchKernelGGL(gi_rowof_kernel, grid, block, 0, s, (const int4*)idx, n, n_dev, v.dims, (const uint2*)v.cells, rowof);
    TODA_LAUNCH_CHECK();
    return TODA_OK;
}

extern "C" int toda_gridindex_from_coords_unordered(const int32_t* idx, int n, const int32_t* n_dev, int batch,
                                                    const int32_t* shape_host, void* gi, int32_t* rowof, int gi_clean,
                                                    void* stream) {
    hipStream_t s = (hipStream_t)stream;
    GiView v;
    int rc = gi_view("gridindex_from_coords_unordered", gi, batch, shape_host, &v);
    if (rc) return rc;
    TODA_CHECK_ARG(n >= 0 && rowof, "gridindex_from_coords_unordered: n < 0 or no rowof");
    if (!gi_clean) {
        TODA_HIP(hipMemsetAsync(v.cells, 0, (size_t)v.n_cells * sizeof(uint2), s));
        TODA_HIP(hipMemsetAsync(v.rowmask, 0, (size_t)v.n_rows, s));
    }
    if (n == 0) return TODA_OK;
    const dim3 grid(cdiv(n, RB_BLOCK)), block(RB_BLOCK);
    // rowof doubles as the "this row set its bit first" flags between mark and alloc (rowof[rank] = row is written last);
    // the total's word is the rank counter
    hipLaunchKernelGGL(gi_mark_first_kernel, grid, block, 0, s, (const int4*)idx, n, n_dev, v.dims, v.cells, v.rowmask, rowof, v.total);
    hipLaunchKernelGGL(gi_alloc_kernel, dim3(cdiv(n, GA_BLOCK)), dim3(GA_BLOCK), 0, s, (const int4*)idx, n, n_dev, v.dims, v.cells,
                       (const int*)rowof, v.total);
    hipLaunchKernelGGL(gi_rowof_kernel, grid, block, 0, s, (const int4*)idx, n, n_dev, v.dims, (const uint2*)v.cells, rowof);
    TODA_LAUNCH_CHECK();
    return TODA_OK;
}

extern "C" int toda_gridindex_clear(const int32_t* idx, int n, const int32_t* n_dev, int batch, const int32_t* shape_host,
                                    void* gi, void* stream) {
    GiView v;
    int rc = gi_view("gridindex_clear", gi, batch, shape_host, &v);
    if (rc) return rc;
    TODA_CHECK_ARG(n >= 0, "gridindex_clear: n < 0");
    if (n == 0) return TODA_OK;
    hipLaunchKernelGGL(gi_clear_kernel, dim3(cdiv(n, RB_BLOCK)), dim3(RB_BLOCK), 0, (hipStream_t)stream, (const int4*)idx, n, n_dev,
                       v.dims, v.cells, v.rowmask);
    TODA_LAUNCH_CHECK();
    return TODA_OK;
}

extern "C" int toda_gridindex_from_conv(const int32_t* idx_in, int n_in, const int32_t* n_in_dev, int batch,
                                        const int32_t* shape_in_host, const int32_t* ksize_host,
                                        const int32_t* stride_host, const int32_t* pad_host,
                                        const int32_t* shape_out_host, void* gi_out, int32_t* idx_out,
                                        int32_t* n_out_dev, int out_cap, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    GiView v;
    ConvGeom cg;
    int rc = conv_setup("gridindex_from_conv", batch, shape_in_host, ksize_host, stride_host, pad_host, shape_out_host, gi_out, &v, &cg);
    if (rc) return rc;
    TODA_CHECK_ARG(n_in >= 0 && out_cap >= 0, "gridindex_from_conv: negative size");
    TODA_HIP(hipMemsetAsync(v.cells, 0, (size_t)v.n_cells * sizeof(uint2), s));
    if (n_in > 0)
        hipLaunchKernelGGL(gi_mark_conv_kernel, dim3(cdiv(n_in, RB_BLOCK)), dim3(RB_BLOCK), 0, s, (const int4*)idx_in,
                           n_in, n_in_dev, cg, v.cells);
    rc = exclusive_scan(CellAccess{v.cells}, v.n_cells, v.part, v.total, s);
    if (rc) return rc;
    hipLaunchKernelGGL(gi_decode_kernel, dim3(cdiv(v.n_cells, RB_BLOCK)), dim3(RB_BLOCK), 0, s, (const uint2*)v.cells, v.n_cells, v.dims,
                       (int4*)idx_out, out_cap, (const int32_t*)v.total, n_out_dev);
    TODA_LAUNCH_CHECK();
    return TODA_OK;
}

extern "C" int toda_gridindex_from_bitmap(const void* gi_in, int batch, const int32_t* shape_in_host,
                                          const int32_t* ksize_host, const int32_t* stride_host, const int32_t* pad_host,
                                          const int32_t* shape_out_host, void* gi_out, int32_t* idx_out, int32_t* n_out_dev,
                                          int out_cap, int in_rows_marked, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    GiView in, out;
    ConvGeom cg;
    int rc = gi_view("gridindex_from_bitmap", gi_in, batch, shape_in_host, &in);
    if (rc) return rc;
    rc = conv_setup("gridindex_from_bitmap", batch, shape_in_host, ksize_host, stride_host, pad_host, shape_out_host, gi_out, &out, &cg);
    if (rc) return rc;
    TODA_CHECK_ARG(out_cap >= 0, "gridindex_from_bitmap: negative size");
    TODA_CHECK_ARG(31 * stride_host[2] + ksize_host[2] <= 32 * CONV_WIN, "gridindex_from_bitmap: x stride %d / kernel %d too wide",
                   stride_host[2], ksize_host[2]);
    const int nb = cdiv(out.n_cells, RB_BLOCK);
    hipLaunchKernelGGL(gi_conv_bits_kernel, dim3(nb), dim3(RB_BLOCK), 0, s, (const uint2*)in.cells,
                       (const unsigned char*)(in_rows_marked ? in.rowmask : nullptr), in.dims, cg, out.cells, out.n_cells, out.part);
    hipLaunchKernelGGL(gi_scan_decode_kernel, dim3(nb), dim3(RB_BLOCK), 0, s, out.cells, out.n_cells, (const int32_t*)out.part, out.dims,
                       (int4*)idx_out, out_cap, out.total, n_out_dev);
    TODA_LAUNCH_CHECK();
    return TODA_OK;
}

extern "C" int toda_rulebook_subm(const int32_t* idx, int n, int batch, const int32_t* shape_host,
                                  const int32_t* ksize_host, const int32_t* dilation_host, const void* gi,
                                  const int32_t* rowof, int32_t* nbr, int32_t* pair_cnt, int cnt_zeroed, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    GiView v;
    int rc = gi_view("rulebook_subm", gi, batch, shape_host, &v);
    if (rc) return rc;
    const int K = ksize_host[0] * ksize_host[1] * ksize_host[2];
    TODA_CHECK_ARG(K >= 1 && K <= 64, "rulebook_subm: kernel volume %d unsupported", K);
    for (int a = 0; a < 3; ++a)
        TODA_CHECK_ARG(ksize_host[a] % 2 == 1 && dilation_host[a] >= 1, "rulebook_subm: kernel must be odd, dilation >= 1");
    if (!cnt_zeroed) TODA_HIP(hipMemsetAsync(pair_cnt, 0, K * sizeof(int32_t), s));
    if (n == 0) return TODA_OK;
    const uint2* cells = v.cells;
    const dim3 grid(cdiv(n, RB_BLOCK)), block(RB_BLOCK);
    if (ksize_host[0] == 3 && ksize_host[1] == 3 && ksize_host[2] == 3)
        hipLaunchKernelGGL(HIP_KERNEL_NAME(rb_subm_kernel<3, 3, 3>), grid, block, 0, s, (const int4*)idx, n, v.dims,
                           dilation_host[0], dilation_host[1], dilation_host[2], cells, rowof, nbr, pair_cnt);
    else
        hipLaunchKernelGGL(rb_subm_generic_kernel, grid, block, 0, s, (const int4*)idx, n, v.dims, ksize_host[0],
                           ksize_host[1], ksize_host[2], dilation_host[0], dilation_host[1], dilation_host[2], cells,
                           rowof, nbr, pair_cnt);
    TODA_LAUNCH_CHECK();
    return TODA_OK;
}

extern "C" int toda_rulebook_conv(const int32_t* idx_in, int n_in, int batch, const int32_t* shape_in_host,
                                  const int32_t* ksize_host, const int32_t* stride_host, const int32_t* pad_host,
                                  const int32_t* shape_out_host, const void* gi_out, int n_out, int32_t* nbr_o2i,
                                  int32_t* nbr_i2o, int32_t* pair_cnt, const int32_t* idx_out, const void* gi_in,
                                  const int32_t* rowof_in, int cnt_zeroed, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    GiView out;
    ConvGeom cg;
    int rc = conv_setup("rulebook_conv", batch, shape_in_host, ksize_host, stride_host, pad_host, shape_out_host, gi_out, &out, &cg);
    if (rc) return rc;
    const int K = ksize_host[0] * ksize_host[1] * ksize_host[2];
    const ConvKernels kernels = conv_kernels(ksize_host);
    // output -> input table by its own output-stationary kernel when the caller has the input level's index and the output
    // coordinates at hand (the index plan does); otherwise 0xFF fill + scattered stores from the input side
    const bool by_output = idx_out && gi_in && kernels.o2i;
    if (!cnt_zeroed) TODA_HIP(hipMemsetAsync(pair_cnt, 0, K * sizeof(int32_t), s));
    if (n_out > 0 && !by_output) TODA_HIP(hipMemsetAsync(nbr_o2i, 0xFF, (size_t)K * n_out * sizeof(int32_t), s));
    const dim3 block(RB_BLOCK);
    if (by_output && n_out > 0) {
        GiView in;
        rc = gi_view("rulebook_conv", gi_in, batch, shape_in_host, &in);
        if (rc) return rc;
        hipLaunchKernelGGL(kernels.o2i, dim3(cdiv(n_out, RB_BLOCK)), block, 0, s, (const int4*)idx_out, n_out, cg, in.dims,
                           (const uint2*)in.cells, rowof_in, n_in, nbr_o2i);
    }
    if (n_in > 0)
        hipLaunchKernelGGL(kernels.i2o, dim3(cdiv(n_in, RB_BLOCK)), block, 0, s, (const int4*)idx_in, n_in, cg, (const uint2*)out.cells,
                           n_out, by_output ? nullptr : nbr_o2i, nbr_i2o, pair_cnt);
    TODA_LAUNCH_CHECK();
    return TODA_OK;
}

