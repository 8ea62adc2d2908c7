// The grid index of one sparse level: the cell word, its rank and the layout of the buffer that holds
// them.  Every translation unit that builds or reads an index takes all three from here.
//
// cell = {32 occupancy bits, rank of the word's first site}; the rank of a set bit is cell.y + popc(cell.x & bits below it): membership
// and row id in one 8-byte load.  With canonical ranks (a popcount scan) the sites are enumerated in ascending
// ((b*D+z)*H+y)*W+x order; the O(sites) builder of the voxel level hands the words' first ranks out in no fixed order instead.
#pragma once
#include "common.h"

namespace toda {

struct GridDims {
    int B, D, H, W;
};

__device__ __forceinline__ long long lin_index(int b, int z, int y, int x, const GridDims& g) {
    return (((long long)b * g.D + z) * g.H + y) * g.W + x;
}

// index of the lattice row (b, z, y) among the row bytes
__device__ __forceinline__ long long row_index(int b, int z, int y, const GridDims& g) {
    return ((long long)b * g.D + z) * g.H + y;
}

__device__ __forceinline__ bool in_lattice(int z, int y, int x, const GridDims& g) {
    return (unsigned)z < (unsigned)g.D && (unsigned)y < (unsigned)g.H && (unsigned)x < (unsigned)g.W;
}

// A coordinate row outside [0,B) x [0,D) x [0,H) x [0,W) (wrong batch_size, coordinates made for another grid, a
// hand-built SparseConvTensor) must never become a bitmap address: such rows are ignored by every builder - they set
// no bit, get no neighbours and are nobody's neighbour.
__device__ __forceinline__ bool in_grid(const int4 c, const GridDims& g) {
    // (the four tests in one flat expression: nested as `batch test && in_lattice(...)` the 27 probes of rb_conv_o2i_kernel<3, 3, 3> compile
    // to 27 branches instead of predicated loads, 1233 -> 1472 instructions, and the kernel measured 4.5 % slower)
    return (unsigned)c.x < (unsigned)g.B && (unsigned)c.y < (unsigned)g.D && (unsigned)c.z < (unsigned)g.H &&
           (unsigned)c.w < (unsigned)g.W;
}

template <class T>
__device__ __forceinline__ int4 lin_coords_as(T t, const GridDims& g) {
    const int x = (int)(t % (T)g.W);
    t /= (T)g.W;
    const int y = (int)(t % (T)g.H);
    t /= (T)g.H;
    return make_int4((int)(t / (T)g.D), (int)(t % (T)g.D), y, x);
}

// the inverse of lin_index: (b, z, y, x) of a linear index.  A lattice of fewer than 2^26 words has every index below 2^31 and
// divides in 32 bits (wave uniform; 64-bit divisions are ~100 instructions each).
__device__ __forceinline__ int4 lin_coords(long long lin, const GridDims& g, long long n_cells) {
    return n_cells < (1LL << 26) ? lin_coords_as((unsigned)lin, g) : lin_coords_as(lin, g);
}

// ---- the cell word ---------------------------------------------------------------------------------------------------------
// {word, bit} of a cell.  A probe that may fail is `cell = {0, 0}, bit = 0; if (inside) gi_fetch(...)` at the call site: a helper that
// took the test as a bool raised rb_conv_o2i_kernel<3, 3, 3> from 94 to 109 VGPRs (5 -> 4 waves).
__device__ __forceinline__ void gi_fetch(const uint2* __restrict__ cells, long long lin, uint2& cell, unsigned& bit) {
    cell = cells[lin >> 5];
    bit = 1u << (lin & 31);
}

// rank of the cell behind a fetched {word, bit}, -1 without a site there; {0, 0} (nothing fetched) ranks as -1, so a table kernel
// issues its K probes as K independent conditional fetches before the first is consumed
__device__ __forceinline__ int gi_rank_of(const uint2 cell, unsigned bit) {
    return (cell.x & bit) ? (int)cell.y + __popc(cell.x & (bit - 1)) : -1;
}

__device__ __forceinline__ int gi_rank(const uint2* __restrict__ cells, long long lin) {
    uint2 cell;
    unsigned bit;
    gi_fetch(cells, lin, cell, bit);
    return gi_rank_of(cell, bit);
}

// set a cell's bit unless it is already visible (plain pre-test: most bits are already set, and once a hot cell's bit is
// visible the atomics stop)
__device__ __forceinline__ void gi_set_bit(uint2* __restrict__ cells, long long lin) {
    const unsigned bit = 1u << (lin & 31);
    unsigned* word = &cells[lin >> 5].x;
    if (!(*word & bit)) atomicOr(word, bit);
}

// set a cell's bit; true for exactly one of several callers with the same cell
__device__ __forceinline__ bool gi_set_bit_first(uint2* __restrict__ cells, long long lin) {
    const unsigned bit = 1u << (lin & 31);
    return !(atomicOr(&cells[lin >> 5].x, bit) & bit);
}

// ---- the buffer ------------------------------------------------------------------------------------------------------------
constexpr int GI_TILE = 256;      // words per partial sum: one block of the bitmap builder (scan.cuh's 2048-word tiles need fewer)

struct GiLayout {
    long long cells;   // number of 32-bit words
    long long rows;    // B * D * H lattice rows (x runs)
    size_t o_cells, o_part, o_total, o_rows, bytes;
};

static GiLayout gi_layout(int batch, const int32_t* shape) {
    GiLayout l;
    long long bits = (long long)batch * shape[0] * shape[1] * shape[2];
    l.cells = (bits + 31) / 32;
    size_t o = 0;
    l.o_cells = o;
    o += align_up((size_t)l.cells * sizeof(uint2), 256);
    l.o_part = o;
    o += align_up((size_t)(cdiv(l.cells, GI_TILE) + 1) * sizeof(int32_t), 256);
    l.o_total = o;
    o += 256;
    // one byte per lattice row (b, z, y): "this row holds a site".  Kept by the O(sites) builder of the voxel level (mark / clear);
    // toda_gridindex_from_bitmap skips the input rows whose byte is zero (most of them at the voxel level: 123 k rows, 46 MB of words)
    l.rows = (long long)batch * shape[0] * shape[1];
    l.o_rows = o;
    o += align_up((size_t)l.rows, 256);
    l.bytes = o;
    return l;
}

// the typed regions of a caller's buffer
struct GiView {
    uint2* cells;
    int32_t* part;             // the scan's partial sums
    int32_t* total;            // number of sites (the unordered builder's rank counter)
    unsigned char* rowmask;
    GridDims dims;
    long long n_cells, n_rows;
};

// checks the lattice, then lays `gi` (which may be null when only the sizes are wanted) out over it
static int gi_view(const char* who, const void* gi, int batch, const int32_t* shape, GiView* v) {
    TODA_CHECK_ARG(batch >= 1 && shape[0] >= 1 && shape[1] >= 1 && shape[2] >= 1, "%s: bad batch/shape", who);
    TODA_CHECK_ARG((long long)batch * shape[0] * shape[1] * shape[2] < (1LL << 36), "%s: lattice too large", who);
    const GiLayout l = gi_layout(batch, shape);
    char* b = (char*)gi;
    v->cells = (uint2*)(b + l.o_cells);
    v->part = (int32_t*)(b + l.o_part);
    v->total = (int32_t*)(b + l.o_total);
    v->rowmask = (unsigned char*)(b + l.o_rows);
    v->dims = GridDims{batch, shape[0], shape[1], shape[2]};
    v->n_cells = l.cells;
    v->n_rows = l.rows;
    return TODA_OK;
}

}  // namespace toda
