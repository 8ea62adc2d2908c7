// Per-object and pyramid augmentations of the point table (reference pcdet/datasets/augmentor/augmentor_utils.py:124-683:
// random_translation_along_*, random_local_translation_along_*, local_rotation, local_scaling, global / local frustum
// dropout, local_pyramid_dropout / _sparsify / _swap) for gfx950.  The reference loops over the boxes in Python and runs
// several full-length numpy passes over the cloud per box; here a point's fate depends only on the point itself and on the
// box list, so one thread carries one point through every box in order.  Both kernels and the column range (a functor of
// points_common.cuh's pt_range_kernel) are single streaming passes over the [n, c] fp32 table (4*n*c bytes in, as much out,
// plus the membership words of the pyramid test).
//
// Roundings follow the reference's numpy code (file built with -ffp-contract=off): the box test is get_points_in_box
// (point_in_box<1>) on the point's current coordinates, translation adds in fp64 and rounds once (equal to the fp32 add for an
// fp32 offset, and to numpy's fp64 add for the world translation's fp64 offset), scaling and rotation are fp32 in the
// reference's operation order, thresholds are compared in fp64.
#include "common.h"
#include "points_common.cuh"

namespace toda {

constexpr int STEP_CHUNK = 64;     // steps staged through LDS at a time
constexpr int STEP_COLS = 10;      // cx cy cz dx dy dz rz op p0 p1
constexpr int PYR_CHUNK = 32;      // pyramids staged at a time = one membership word

enum StepOp { OP_TX = 0, OP_TY, OP_TZ, OP_ROT, OP_SCALE, OP_DROP_Z_GE, OP_DROP_Z_LE, OP_DROP_Y_GE, OP_DROP_Y_LE, OP_COUNT, OP_WORLD = 16 };

struct StepPre {
    BoxPre b;
    double p0;
    float p1;
    int op;
};

// One thread per row: load it once, walk the step table in order (LDS chunks of STEP_CHUNK, the loop is uniform over the
// wave), test the current coordinates against the step's box and apply its op on a hit.  A dropped row takes no further
// part.  Rows in [rows, n) are copied so that dst is complete when it does not alias src.
__global__ void __launch_bounds__(PT_BLOCK)
points_box_steps_kernel(const float* src, int n, const int32_t* __restrict__ n_dev, int c, const double* __restrict__ steps,
                        int n_steps, float* dst, int32_t* __restrict__ keep) {   // dst may alias src
    __shared__ StepPre ss[STEP_CHUNK];
    const int j = pt_row(n, nullptr);                     // rows in [min(n, *n_dev), n) are not active
    const bool active = pt_row(n, n_dev) >= 0;
    float x = 0.f, y = 0.f, z = 0.f;
    if (active) x = src[(size_t)j * c], y = src[(size_t)j * c + 1], z = src[(size_t)j * c + 2];
    bool alive = active;
    for (int base = 0; base < n_steps; base += STEP_CHUNK) {
        const int m = n_steps - base < STEP_CHUNK ? n_steps - base : STEP_CHUNK;
        __syncthreads();
        if ((int)threadIdx.x < m) {
            const double* r = steps + (size_t)(base + threadIdx.x) * STEP_COLS;
            StepPre s;
            s.b.cx = (float)r[0], s.b.cy = (float)r[1], s.b.cz = (float)r[2];
            s.b.dx = (float)r[3], s.b.dy = (float)r[4], s.b.dz = (float)r[5];
            const double a = (double)(-(float)r[6]);
            s.b.cosa = (float)cos(a);
            s.b.sina = (float)sin(a);
            s.op = (int)r[7], s.p0 = r[8], s.p1 = (float)r[9];
            ss[threadIdx.x] = s;
        }
        __syncthreads();
        for (int i = 0; i < m; ++i) {
            const StepPre& s = ss[i];
            if (!alive) continue;
            if (!(s.op & OP_WORLD) && !point_in_box<1>(x, y, z, s.b)) continue;
            switch (s.op & 15) {
            case OP_TX: x = (float)((double)x + s.p0); break;
            case OP_TY: y = (float)((double)y + s.p0); break;
            case OP_TZ: z = (float)((double)z + s.p0); break;
            case OP_ROT: {           // about the box centre; row vector times [[c, s], [-s, c]] as rotate_points_along_z
                const float cs = (float)s.p0, sn = s.p1;
                const float sx = x - s.b.cx, sy = y - s.b.cy, sz = z - s.b.cz;
                const float nx = sx * cs + sy * (-sn);
                const float ny = sx * sn + sy * cs;
                x = nx + s.b.cx, y = ny + s.b.cy, z = sz + s.b.cz;
                break;
            }
            case OP_SCALE: {
                const float f = (float)s.p0;
                x = (x - s.b.cx) * f + s.b.cx;
                y = (y - s.b.cy) * f + s.b.cy;
                z = (z - s.b.cz) * f + s.b.cz;
                break;
            }
            case OP_DROP_Z_GE: alive = !((double)z >= s.p0); break;
            case OP_DROP_Z_LE: alive = !((double)z <= s.p0); break;
            case OP_DROP_Y_GE: alive = !((double)y >= s.p0); break;
            case OP_DROP_Y_LE: alive = !((double)y <= s.p0); break;
            default: break;
            }
        }
    }
    if (j < 0) return;
    const float* p = src + (size_t)j * c;
    float* q = dst + (size_t)j * c;
    if (active) {
        q[0] = x, q[1] = y, q[2] = z;
        if (q != p)
            for (int ch = 3; ch < c; ++ch) q[ch] = p[ch];
    } else if (q != p) {
        for (int ch = 0; ch < c; ++ch) q[ch] = p[ch];
    }
    if (keep) keep[j] = alive ? 1 : 0;
}

// the value of pt_range_kernel (points_common.cuh) for a column's min / max: every valid row counts.  On a cloud that holds NaN
// the threshold formed from this range is not numpy's (fminf / fmaxf skip a NaN).
struct ColumnOfRow {
    int col;
    __device__ bool operator()(const float* __restrict__ p, float& v) const {
        v = p[col];
        return true;
    }
};

// five half-spaces n . p <= d with outward normals: the four sides through the apex, then the base
struct PyrPre {
    double nx[5], ny[5], nz[5], d[5];
};

// pyramid = apex, base corner 0..3 (get_pyramids' [5, 3] layout, the base corners in order round the face)
__device__ __forceinline__ PyrPre pyramid_planes(const double* __restrict__ v) {
    PyrPre r;
    const double gx = (v[0] + v[3] + v[6] + v[9] + v[12]) / 5.0, gy = (v[1] + v[4] + v[7] + v[10] + v[13]) / 5.0,
                 gz = (v[2] + v[5] + v[8] + v[11] + v[14]) / 5.0;
    for (int f = 0; f < 5; ++f) {
        // face f < 4: apex, corner f, corner f + 1;  face 4: corner 0, corner 1, corner 3
        const double* a = f < 4 ? v : v + 3;
        const double* b = f < 4 ? v + 3 * (1 + f) : v + 6;
        const double* e = f < 4 ? v + 3 * (1 + (f + 1) % 4) : v + 12;
        const double ux = b[0] - a[0], uy = b[1] - a[1], uz = b[2] - a[2];
        const double wx = e[0] - a[0], wy = e[1] - a[1], wz = e[2] - a[2];
        double nx = uy * wz - uz * wy, ny = uz * wx - ux * wz, nz = ux * wy - uy * wx;
        if (nx * (gx - a[0]) + ny * (gy - a[1]) + nz * (gz - a[2]) > 0.0) nx = -nx, ny = -ny, nz = -nz;
        r.nx[f] = nx, r.ny[f] = ny, r.nz[f] = nz;
        r.d[f] = nx * a[0] + ny * a[1] + nz * a[2];
    }
    return r;
}

// Membership of every row in every pyramid: bits[j, w] bit q = row j lies in pyramid 32 w + q; counts[p] = rows in pyramid p
// (integer atomics: one LDS add per wave and pyramid, one global add per workgroup and pyramid - deterministic).
__global__ void __launch_bounds__(PT_BLOCK)
points_in_pyramids_kernel(const float* __restrict__ pts, int n, const int32_t* __restrict__ n_dev, int c,
                          const double* __restrict__ pyramids, int np, int words, uint32_t* __restrict__ bits,
                          int32_t* __restrict__ counts) {
    __shared__ PyrPre sp[PYR_CHUNK];
    __shared__ int scnt[PYR_CHUNK];
    const int j = pt_row(n, nullptr);                     // rows in [min(n, *n_dev), n) are not active
    const bool active = pt_row(n, n_dev) >= 0;
    double x = 0.0, y = 0.0, z = 0.0;
    if (active) x = (double)pts[(size_t)j * c], y = (double)pts[(size_t)j * c + 1], z = (double)pts[(size_t)j * c + 2];
    for (int w = 0; w < words; ++w) {
        const int m = np - w * PYR_CHUNK < PYR_CHUNK ? np - w * PYR_CHUNK : PYR_CHUNK;
        __syncthreads();
        if ((int)threadIdx.x < PYR_CHUNK) scnt[threadIdx.x] = 0;
        if ((int)threadIdx.x < m) sp[threadIdx.x] = pyramid_planes(pyramids + (size_t)(w * PYR_CHUNK + threadIdx.x) * 15);
        __syncthreads();
        uint32_t word = 0;
        for (int q = 0; q < m; ++q) {
            const PyrPre& p = sp[q];
            bool in = active;
            for (int f = 0; f < 5; ++f) in = in && (p.nx[f] * x + p.ny[f] * y + p.nz[f] * z <= p.d[f]);
            word |= (in ? 1u : 0u) << q;
            const int cnt = __popcll(__ballot(in));
            if ((threadIdx.x & 63) == 0 && cnt) atomicAdd(&scnt[q], cnt);
        }
        if (j >= 0) bits[(size_t)j * words + w] = word;
        __syncthreads();
        if ((int)threadIdx.x < m && scnt[threadIdx.x]) atomicAdd(&counts[w * PYR_CHUNK + threadIdx.x], scnt[threadIdx.x]);
    }
}

}  // namespace toda

using namespace toda;

extern "C" int toda_points_box_steps_chunk(void) { return STEP_CHUNK; }

extern "C" int toda_points_box_steps(const float* src, int n, const int32_t* n_dev, int c, const double* steps, int n_steps,
                                     float* dst, int32_t* keep, void* stream) {
    PT_CHECK_SIZES("points_box_steps");
    TODA_CHECK_ARG(n_steps >= 0, "points_box_steps: n_steps >= 0");
    PT_CHECK_TABLES(src && dst && (steps || n_steps == 0), "points_box_steps: null table");
    hipLaunchKernelGGL(points_box_steps_kernel, dim3(cdiv(n, PT_BLOCK)), dim3(PT_BLOCK), 0, (hipStream_t)stream, src, n, n_dev, c, steps,
                       n_steps, dst, keep);
    TODA_LAUNCH_CHECK();
    return TODA_OK;
}

extern "C" size_t toda_points_column_range_workspace_bytes(void) { return pt_range_workspace_bytes(); }

extern "C" int toda_points_column_range(const float* points, int n, const int32_t* n_dev, int c, int col, float* range_dev,
                                        void* ws, size_t ws_bytes, void* stream) {
    TODA_CHECK_ARG(n >= 0 && c >= 1 && col >= 0 && col < c, "points_column_range: need n >= 0 and a column in [0, c)");
    return pt_range_pass("points_column_range", points, n, n_dev, c, ColumnOfRow{col}, range_dev, ws, ws_bytes, stream);
}

extern "C" int toda_points_in_pyramids(const float* points, int n, const int32_t* n_dev, int c, const double* pyramids, int np,
                                       uint32_t* bits, int32_t* counts, void* stream) {
    PT_CHECK_SIZES("points_in_pyramids");
    TODA_CHECK_ARG(np >= 0, "points_in_pyramids: pyramid count >= 0");
    if (np == 0) return TODA_OK;
    PT_CHECK_TABLES(points && pyramids && bits && counts, "points_in_pyramids: null table");
    hipStream_t s = (hipStream_t)stream;
    TODA_HIP(hipMemsetAsync(counts, 0, (size_t)np * sizeof(int32_t), s));
    hipLaunchKernelGGL(points_in_pyramids_kernel, dim3(cdiv(n, PT_BLOCK)), dim3(PT_BLOCK), 0, s, points, n, n_dev, c, pyramids, np,
                       cdiv(np, PYR_CHUNK), bits, counts);
    TODA_LAUNCH_CHECK();
    return TODA_OK;
}
