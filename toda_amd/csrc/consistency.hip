// The consistency term of the stage-2 step for gfx950 (reference pcdet/models/__init__.py get_consistency_loss, :216-260): mutual
// nearest-centre matching between the boxes of the two passes and both loss terms, for the whole batch in two launches.  The
// reference forms the [Na, No, 3] difference tensor per sample and reduces it twice; here a row keeps its running (best, index)
// in registers while the other side passes through LDS, so nothing of size Na x No exists anywhere.
//
//   cons_match   grid (row tiles, 2 directions, batch), CONS_BLOCK threads, one row per thread.  Direction 0: a row is an adv
//                box and looks for its org partner; direction 1 the other way round.  The other side is staged through LDS in
//                chunks of CONS_BLOCK x (x, y, z, selected); every lane reads the same LDS word (a broadcast), eight reads in
//                flight.  A matched row gathers its partner's six floats from global memory.  The block's two sums and two counts go to
//                ws[(b * 2 + dir) * tiles + tile]: lanes by a width-64 butterfly, the four waves in wave order through LDS.
//   cons_fold    one workgroup: thread b folds sample b's partials in (direction, tile) order, then thread 0 folds the samples
//                in index order and divides.
//
// Arithmetic (-ffp-contract=off): d2 = ((ax - ox)^2 + (ay - oy)^2) + (az - oz)^2 in fp32.  torch.min's rule for NaN: a NaN
// distance is smaller than every number, and the first one met stays.  No float atomics; every fold has one fixed order, so
// two runs give the same bits.  The chain of fp32 additions a term passes through: 2 inside the row, 6 butterfly levels, 3
// across the waves, 2 * tiles in cons_fold, then one per sample of the batch.
#include "common.h"

namespace toda {

constexpr int CONS_BLOCK = 256;
constexpr int CONS_WAVE = 64;              // gfx950: wavefronts of 64 lanes
constexpr int CONS_WAVES = CONS_BLOCK / CONS_WAVE;
static_assert(CONS_BLOCK % CONS_WAVE == 0, "cons_match_kernel folds whole waves");

struct ConsPartial {
    float centre, size;
    int32_t selected, matched;
};

__device__ __forceinline__ float cons_wave_sum(float v) {
#pragma unroll
    for (int m = CONS_WAVE / 2; m >= 1; m >>= 1) v += __shfl_xor(v, m, CONS_WAVE);
    return v;
}

__global__ void __launch_bounds__(CONS_BLOCK)
cons_match_kernel(const float* __restrict__ adv, const uint8_t* __restrict__ adv_sel, int na, const float* __restrict__ org,
                  const uint8_t* __restrict__ org_sel, int no, int cols, float match_dist2, ConsPartial* __restrict__ partials) {
    __shared__ float4 stage[CONS_BLOCK];
    __shared__ ConsPartial swave[CONS_WAVES];
    const int t = threadIdx.x, dir = blockIdx.y, b = blockIdx.z;
    const int nr = dir == 0 ? na : no, nc = dir == 0 ? no : na;
    const float* rows = (dir == 0 ? adv : org) + (size_t)b * nr * cols;
    const float* opp = (dir == 0 ? org : adv) + (size_t)b * nc * cols;
    const uint8_t* rsel = (dir == 0 ? adv_sel : org_sel) + (size_t)b * nr;
    const uint8_t* osel = (dir == 0 ? org_sel : adv_sel) + (size_t)b * nc;

    const int r = blockIdx.x * CONS_BLOCK + t;
    const bool valid = r < nr && rsel[r] != 0;
    float x = 0.f, y = 0.f, z = 0.f;
    if (valid) x = rows[(size_t)r * cols], y = rows[(size_t)r * cols + 1], z = rows[(size_t)r * cols + 2];
    float best = __builtin_inff();
    int idx = -1;
    for (int base = 0; base < nc; base += CONS_BLOCK) {
        __syncthreads();
        float4 s = make_float4(0.f, 0.f, 0.f, 0.f);             // past the end or unselected: never read, w = 0
        if (base + t < nc && osel[base + t] != 0) {
            const float* q = opp + (size_t)(base + t) * cols;
            s = make_float4(q[0], q[1], q[2], 1.f);
        }
        stage[t] = s;
        __syncthreads();
        // a whole chunk every time and no branch on w, so eight broadcast reads are in flight at once; an entry with w = 0 stands at
        // +inf, which is below no running best
#pragma unroll 8
        for (int j = 0; j < CONS_BLOCK; ++j) {
            const float4 o = stage[j];
            const float dx = x - o.x, dy = y - o.y, dz = z - o.z;
            float d = (dx * dx + dy * dy) + dz * dz;
            d = o.w != 0.f ? d : __builtin_inff();
            if (!(best != best) && (d < best || d != d)) best = d, idx = base + j;
        }
    }
    const bool matched = valid && idx >= 0 && best < match_dist2;
    float centre = 0.f, size = 0.f;
    if (matched) {
        const float* p = rows + (size_t)r * cols;
        const float* q = opp + (size_t)idx * cols;
        const float c0 = fabsf(p[0] - q[0]), c1 = fabsf(p[1] - q[1]), c2 = fabsf(p[2] - q[2]);
        const float s0 = p[3] - q[3], s1 = p[4] - q[4], s2 = p[5] - q[5];
        centre = (c0 + c1) + c2;
        size = (s0 * s0 + s1 * s1) + s2 * s2;
    }
    centre = cons_wave_sum(centre);
    size = cons_wave_sum(size);
    const int n_sel = __popcll(__ballot(valid)), n_match = __popcll(__ballot(matched));
    if ((t & (CONS_WAVE - 1)) == 0) {
        ConsPartial w;
        w.centre = centre, w.size = size, w.selected = n_sel, w.matched = n_match;
        swave[t / CONS_WAVE] = w;
    }
    __syncthreads();
    if (t == 0) {
        ConsPartial acc = swave[0];
        for (int w = 1; w < CONS_WAVES; ++w) {
            acc.centre += swave[w].centre, acc.size += swave[w].size;
            acc.selected += swave[w].selected, acc.matched += swave[w].matched;
        }
        partials[((size_t)b * 2 + dir) * gridDim.x + blockIdx.x] = acc;
    }
}

// out[2 + 4 b ..]: centre_sum, size_sum, selected, matched of sample b; out[0], out[1]: the batch means of the per-sample terms
__global__ void __launch_bounds__(CONS_WAVE)
cons_fold_kernel(const ConsPartial* __restrict__ partials, int tiles, int batch, float* __restrict__ out) {
    for (int b = threadIdx.x; b < batch; b += CONS_WAVE) {
        const ConsPartial* p = partials + (size_t)b * 2 * tiles;
        ConsPartial acc = p[0];
        for (int k = 1; k < 2 * tiles; ++k) {
            acc.centre += p[k].centre, acc.size += p[k].size;
            acc.selected += p[k].selected, acc.matched += p[k].matched;
        }
        float* o = out + 2 + (size_t)b * 4;
        o[0] = acc.centre, o[1] = acc.size, o[2] = (float)acc.selected, o[3] = (float)acc.matched;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float centre = 0.f, size = 0.f;
        for (int b = 0; b < batch; ++b) {
            const float* o = out + 2 + (size_t)b * 4;
            const float n = o[2] > 1.f ? o[2] : 1.f;
            centre += o[0] / n, size += o[1] / n;
        }
        out[0] = centre / (float)batch, out[1] = size / (float)batch;
    }
}

static int cons_tiles(int na, int no) {
    const int rows = na > no ? na : no;
    return rows > 0 ? cdiv(rows, CONS_BLOCK) : 1;
}

}  // namespace toda

using namespace toda;

extern "C" size_t toda_consistency_workspace_bytes(int batch, int na, int no) {
    if (batch < 1 || na < 0 || no < 0) return 0;
    return align_up((size_t)batch * 2 * cons_tiles(na, no) * sizeof(ConsPartial), 256);
}

extern "C" int toda_consistency_loss(const float* adv, const uint8_t* adv_sel, int na, const float* org, const uint8_t* org_sel,
                                     int no, int batch, int cols, float match_dist2, float* out, void* ws, size_t ws_bytes,
                                     void* stream) {
    TODA_CHECK_ARG(batch >= 1 && batch <= 65535, "consistency_loss: need 1 <= batch <= 65535, got %d", batch);
    TODA_CHECK_ARG(na >= 0 && no >= 0, "consistency_loss: need na >= 0 and no >= 0 rows, got %d and %d", na, no);
    TODA_CHECK_ARG(cols >= 6, "consistency_loss: need at least 6 columns (x y z dx dy dz), got %d", cols);
    const size_t need = toda_consistency_workspace_bytes(batch, na, no);
    if (ws_bytes < need) {
        set_error("consistency_loss: workspace %zu < required %zu", ws_bytes, need);
        return TODA_EWORKSPACE;
    }
    TODA_CHECK_ARG(out && ws, "consistency_loss: null out or workspace");
    TODA_CHECK_ARG((adv && adv_sel) || na == 0, "consistency_loss: null adv boxes or selection with na = %d", na);
    TODA_CHECK_ARG((org && org_sel) || no == 0, "consistency_loss: null org boxes or selection with no = %d", no);
    hipStream_t s = (hipStream_t)stream;
    const int tiles = cons_tiles(na, no);
    ConsPartial* partials = (ConsPartial*)ws;
    hipLaunchKernelGGL(cons_match_kernel, dim3(tiles, 2, batch), dim3(CONS_BLOCK), 0, s, adv, adv_sel, na, org, org_sel, no, cols,
                       match_dist2, partials);
    hipLaunchKernelGGL(cons_fold_kernel, dim3(1), dim3(CONS_WAVE), 0, s, (const ConsPartial*)partials, tiles, batch, out);
    TODA_LAUNCH_CHECK();
    return TODA_OK;
}
