// VoxelRCNNHead's device side for gfx950: the voxel query and the fused neighbour pool of NeighborVoxelSAModuleMSG
// (reference pcdet/ops/pointnet2/pointnet2_stack/src/voxel_query_gpu.cu, voxel_query_utils.py:10-103,
// voxel_pool_modules.py:80-131).
//
// toda_voxel_query: one lane per grid point scans its (2 rz + 1)(2 ry + 1)(2 rx + 1) lattice neighbours dz, then dy, then dx,
// skips coordinates off the lattice, looks membership and row up in the level's grid index (bitmap + popcount rank, then rowof
// when the rows are not in canonical order) instead of a dense [B, Z, Y, X] table, and keeps the neighbours whose voxel centre
// lies within the radius, in scan order.  The first hit fills the whole row, later hits overwrite slots 1.. nsample - 1; the
// scan stops at nsample hits (later hits change nothing).  Empty ball: row of zeros and the flag.  dist2 is evaluated in fp32
// in the reference's order; the file is compiled with contraction off, so the radius decisions equal a torch restatement.
//
// The pool.  The reference builds [M, C, nsample] tensors (grouped features, grouped xyz, position features, their sum, the
// ReLU) and max-pools over nsample.  mlps_pos (Conv2d 3 -> C, BatchNorm2d) acts on relative positions that carry no gradient,
// so it folds into a per-channel affine map a_c . d + b_c computed on the host side from the moments of d
// (toda_voxel_pool_moments: mean and biased covariance over all M x nsample entries, fp64, fixed-order fold).  The forward then
// reads every neighbour row once: out[m, c] = max_s relu(f[idx[m, s], c] [not empty] + a_c . d_ms + b_c), with the first
// arg-max s stored as a byte (0xff where the maximum is 0, i.e. no gradient passes the ReLU).
// Backward: d f through the inverse neighbour table, one lane per (row, channel) summing its entries in table order; d a, d b as
// per-workgroup fp64 partials folded in a fixed order (pool_common.cuh).  No float atomics: every result is bit-reproducible.
// The table (toda_voxel_pool_table, the name kept for ABI stability; per row its (m, s) entries ascending: integer counts, a scan
// and the stable sort of radix_sort.cuh) also serves the SA gather's d P and the BEV interpolation's d map (pointnet2_stack.hip).
#include "grid_index.cuh"
#include "pool_common.cuh"
#include "radix_sort.cuh"

namespace toda {

constexpr int VQ_BLOCK = 256;
constexpr int VP_BLOCK = 256;
constexpr int VP_POINTS = 16;          // grid points per forward workgroup
constexpr int VP_MAX_NSAMPLE = 64;
constexpr int VP_ARG_NONE = 0xff;
constexpr int VM_BLOCKS = 256;         // moment partials (fixed: the fold order depends on nothing but M)
constexpr int VB_LANES = 4;            // row lanes per d a / d b workgroup (x 64 channels)
constexpr int VB_BLOCKS = 256;

struct VqGeom {
    GridDims grid;
    int rz, ry, rx;
    int nsample;
    float radius2;
};

__global__ void __launch_bounds__(VQ_BLOCK)
voxel_query_kernel(const float* __restrict__ new_xyz, const int4* __restrict__ new_coords, int M, const float* __restrict__ xyz, int N,
                   const uint2* __restrict__ cells, const int* __restrict__ rowof, VqGeom g, int* __restrict__ idx,
                   uint8_t* __restrict__ empty) {
    const int m = blockIdx.x * VQ_BLOCK + threadIdx.x;
    if (m >= M) return;
    const int4 c = new_coords[m];            // (b, z, y, x)
    const float nx = new_xyz[(size_t)m * 3 + 0], ny = new_xyz[(size_t)m * 3 + 1], nz = new_xyz[(size_t)m * 3 + 2];
    int* out = idx + (size_t)m * g.nsample;
    int cnt = 0;
    if ((unsigned)c.x < (unsigned)g.grid.B) {
        for (int dz = -g.rz; dz <= g.rz && cnt < g.nsample; ++dz) {
            const int z = c.y + dz;
            if (z < 0 || z >= g.grid.D) continue;
            for (int dy = -g.ry; dy <= g.ry && cnt < g.nsample; ++dy) {
                const int y = c.z + dy;
                if (y < 0 || y >= g.grid.H) continue;
                for (int dx = -g.rx; dx <= g.rx && cnt < g.nsample; ++dx) {
                    const int x = c.w + dx;
                    if (x < 0 || x >= g.grid.W) continue;
                    int row = gi_rank(cells, lin_index(c.x, z, y, x, g.grid));
                    if (row < 0) continue;
                    if (rowof) row = rowof[row];
                    if ((unsigned)row >= (unsigned)N) continue;
                    const float ex = xyz[(size_t)row * 3 + 0] - nx, ey = xyz[(size_t)row * 3 + 1] - ny, ez = xyz[(size_t)row * 3 + 2] - nz;
                    const float dist2 = ex * ex + ey * ey + ez * ez;
                    if (dist2 > g.radius2) continue;
                    if (cnt == 0)
                        for (int l = 1; l < g.nsample; ++l) out[l] = row;
                    out[cnt++] = row;
                }
            }
        }
    }
    if (cnt == 0)
        for (int l = 0; l < g.nsample; ++l) out[l] = 0;
    empty[m] = cnt == 0;
}

__device__ __forceinline__ void block_sum_doubles(double* v, int nv, double* s_red) {
    // fixed-order tree over the 256 lanes of the block, nv values per lane; result in lane 0's v
    for (int k = 0; k < nv; ++k) s_red[k * VP_BLOCK + threadIdx.x] = v[k];
    __syncthreads();
    for (int w = VP_BLOCK / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w)
            for (int k = 0; k < nv; ++k) s_red[k * VP_BLOCK + threadIdx.x] += s_red[k * VP_BLOCK + threadIdx.x + w];
        __syncthreads();
    }
    for (int k = 0; k < nv; ++k) v[k] = s_red[k * VP_BLOCK];
}

// partial sums of d (3) and d d^T (6: xx xy xz yy yz zz) per workgroup, entries in a fixed assignment to lanes
__global__ void __launch_bounds__(VP_BLOCK)
voxel_pool_moments_kernel(const int* __restrict__ idx, const uint8_t* __restrict__ empty, int M, int ns, const float* __restrict__ xyz, int N,
                          const float* __restrict__ new_xyz, double* __restrict__ part) {
    __shared__ double s_red[9 * VP_BLOCK];
    double v[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    const long long E = (long long)M * ns;
    for (long long e = (long long)blockIdx.x * VP_BLOCK + threadIdx.x; e < E; e += (long long)gridDim.x * VP_BLOCK) {
        const int m = (int)(e / ns);
        float d[3];
        rel_delta(xyz, new_xyz, idx[e], N, m, empty[m] != 0, d);
        const double x = d[0], y = d[1], z = d[2];
        v[0] += x; v[1] += y; v[2] += z;
        v[3] += x * x; v[4] += x * y; v[5] += x * z; v[6] += y * y; v[7] += y * z; v[8] += z * z;
    }
    block_sum_doubles(v, 9, s_red);
    if (threadIdx.x == 0)
        for (int k = 0; k < 9; ++k) part[(size_t)blockIdx.x * 9 + k] = v[k];
}

// one lane per moment, blocks in order; out = mean (3) + biased covariance (9, row-major)
__global__ void voxel_pool_moments_fold_kernel(const double* __restrict__ part, int nblk, long long E, double* __restrict__ out) {
    __shared__ double s[9];
    const int k = threadIdx.x;
    if (k < 9) {
        double acc = 0.0;
        for (int b = 0; b < nblk; ++b) acc += part[(size_t)b * 9 + k];
        s[k] = acc / (double)E;
    }
    __syncthreads();
    if (k < 3) out[k] = s[k];
    if (k < 9) {
        const int i = k / 3, j = k % 3;
        const int lo = i < j ? i : j, hi = i < j ? j : i;
        const int q = lo == 0 ? 3 + hi : (lo == 1 ? 5 + hi : 8);      // xx xy xz | yy yz | zz
        out[3 + k] = s[q] - s[i] * s[j];
    }
}

// workgroup: VP_POINTS grid points; their rows and relative positions staged in LDS, lanes over (point, channel), channel fastest
__global__ void __launch_bounds__(VP_BLOCK)
voxel_pool_fwd_kernel(const float* __restrict__ f, int N, int C, const int* __restrict__ idx, const uint8_t* __restrict__ empty, int M,
                      int ns, const float* __restrict__ xyz, const float* __restrict__ new_xyz, const float4* __restrict__ ab,
                      float* __restrict__ out, uint8_t* __restrict__ arg) {
    __shared__ int s_row[VP_POINTS * VP_MAX_NSAMPLE];
    __shared__ float s_d[VP_POINTS * VP_MAX_NSAMPLE * 3];
    const int m0 = blockIdx.x * VP_POINTS;
    const int np = min(VP_POINTS, M - m0);
    for (int i = threadIdx.x; i < np * ns; i += VP_BLOCK) {
        const int m = m0 + i / ns;
        const bool e = empty[m] != 0;
        const int row = idx[(size_t)m * ns + i % ns];
        float d[3];
        rel_delta(xyz, new_xyz, row, N, m, e, d);
        s_row[i] = (!e && (unsigned)row < (unsigned)N) ? row : -1;
        s_d[i * 3 + 0] = d[0];
        s_d[i * 3 + 1] = d[1];
        s_d[i * 3 + 2] = d[2];
    }
    __syncthreads();
    for (int i = threadIdx.x; i < np * C; i += VP_BLOCK) {
        const int p = i / C, c = i % C;
        const float4 w = ab[c];
        float best = 0.0f;
        int at = 0;
        for (int s = 0; s < ns; ++s) {
            const int q = p * ns + s;
            const int row = s_row[q];
            const float fe = row >= 0 ? f[(size_t)row * C + c] : 0.0f;
            const float pos = w.x * s_d[q * 3 + 0] + w.y * s_d[q * 3 + 1] + w.z * s_d[q * 3 + 2] + w.w;
            const float r = fmaxf(fe + pos, 0.0f);
            if (s == 0 || r > best) {
                best = r;
                at = s;
            }
        }
        const size_t o = (size_t)(m0 + p) * C + c;
        out[o] = best;
        if (arg) arg[o] = best > 0.0f ? (uint8_t)at : (uint8_t)VP_ARG_NONE;
    }
}

// inverse table, step 1: key = row of the entry (N for an empty ball), val = entry; integer counts per row
__global__ void __launch_bounds__(VP_BLOCK)
voxel_pool_keys_kernel(const int* __restrict__ idx, const uint8_t* __restrict__ empty, int M, int ns, int N, int32_t* __restrict__ key,
                       int32_t* __restrict__ val, int32_t* __restrict__ cnt) {
    const long long e = (long long)blockIdx.x * VP_BLOCK + threadIdx.x;
    if (e >= (long long)M * ns) return;
    const int row = idx[e];
    const bool ok = !empty[e / ns] && (unsigned)row < (unsigned)N;
    key[e] = ok ? row : N;
    val[e] = (int)e;
    if (ok) atomicAdd(&cnt[row], 1);
}

// d f[n, c] = sum over the entries (m, s) of row n, in table order, of g[m, c] where s is the stored arg-max
__global__ void __launch_bounds__(VP_BLOCK)
voxel_pool_bwd_feat_kernel(const float* __restrict__ g, const uint8_t* __restrict__ arg, int ns, int C, const int32_t* __restrict__ off,
                           const int32_t* __restrict__ ent, int N, float* __restrict__ gf) {
    const long long i = (long long)blockIdx.x * VP_BLOCK + threadIdx.x;
    if (i >= (long long)N * C) return;
    const int n = (int)(i / C), c = (int)(i % C);
    float acc = 0.0f;
    for (int j = off[n], end = off[n + 1]; j < end; ++j) {
        const int e = ent[j];
        const int m = e / ns, s = e % ns;
        const size_t o = (size_t)m * C + c;
        if (arg[o] == s) acc += g[o];
    }
    gf[i] = acc;
}

// d b[c] = sum_m g[m, c] [gradient passes], d a[c] = sum_m g[m, c] d_{m, arg}: lanes (row lane, channel), fp64, fixed rows per lane
__global__ void __launch_bounds__(VP_BLOCK)
voxel_pool_bwd_pos_kernel(const float* __restrict__ g, const uint8_t* __restrict__ arg, const int* __restrict__ idx,
                          const uint8_t* __restrict__ empty, int M, int ns, int C, const float* __restrict__ xyz, int N,
                          const float* __restrict__ new_xyz, double* __restrict__ part) {
    __shared__ double s_red[4][VP_BLOCK];
    const int lane = threadIdx.x / 64, c = blockIdx.y * 64 + (threadIdx.x & 63);
    double v[4] = {0, 0, 0, 0};
    if (c < C) {
        for (int m = blockIdx.x * VB_LANES + lane; m < M; m += gridDim.x * VB_LANES) {
            const size_t o = (size_t)m * C + c;
            const int s = arg[o];
            if (s == VP_ARG_NONE || s >= ns) continue;
            const double gv = g[o];
            float d[3];
            rel_delta(xyz, new_xyz, idx[(size_t)m * ns + s], N, m, empty[m] != 0, d);
            v[0] += gv * d[0];
            v[1] += gv * d[1];
            v[2] += gv * d[2];
            v[3] += gv;
        }
    }
    for (int k = 0; k < 4; ++k) s_red[k][threadIdx.x] = v[k];
    __syncthreads();
    if (lane == 0 && c < C) {
        for (int k = 0; k < 4; ++k) {
            double acc = s_red[k][threadIdx.x];
            for (int l = 1; l < VB_LANES; ++l) acc += s_red[k][l * 64 + threadIdx.x];
            part[((size_t)blockIdx.x * C + c) * 4 + k] = acc;
        }
    }
}

struct VtLayout {
    RsLayout sort;
    size_t scan_part, bytes;
};

static VtLayout vt_layout(int M, int ns, int N) {
    VtLayout l;
    l.sort = rs_layout((long long)M * ns, 0);
    l.scan_part = l.sort.end;
    l.bytes = l.scan_part + scan_partials_bytes((long long)N + 1);
    return l;
}

}  // namespace toda

using namespace toda;

extern "C" int toda_voxel_query(const float* new_xyz, const int32_t* new_coords, int M, const float* xyz, int N, const void* gi,
                                const int32_t* rowof, int batch, const int32_t* shape_host, float radius, const int32_t* ranges_host,
                                int nsample, int32_t* idx, uint8_t* empty, void* stream) {
    TODA_CHECK_ARG(M >= 0 && N >= 0 && batch >= 1, "voxel_query: M=%d N=%d batch=%d", M, N, batch);
    TODA_CHECK_ARG(nsample >= 1 && nsample <= VP_MAX_NSAMPLE, "voxel_query: nsample %d outside [1, %d]", nsample, VP_MAX_NSAMPLE);
    TODA_CHECK_ARG(shape_host && ranges_host, "voxel_query: shape and query ranges are required");
    TODA_CHECK_ARG(shape_host[0] >= 1 && shape_host[1] >= 1 && shape_host[2] >= 1, "voxel_query: lattice shape must be positive");
    TODA_CHECK_ARG(ranges_host[0] >= 0 && ranges_host[1] >= 0 && ranges_host[2] >= 0 && ranges_host[0] <= 64 && ranges_host[1] <= 64 &&
                       ranges_host[2] <= 64,
                   "voxel_query: query ranges must lie in [0, 64]");
    TODA_CHECK_ARG(radius >= 0.0f, "voxel_query: radius must be >= 0");
    TODA_CHECK_ARG((long long)M * nsample < (1LL << 31), "voxel_query: M x nsample too large");
    if (M == 0) return TODA_OK;
    TODA_CHECK_ARG(new_xyz && new_coords && gi && idx && empty && (N == 0 || xyz), "voxel_query: null pointer");
    GiView v;
    int rc = gi_view("voxel_query", gi, batch, shape_host, &v);
    if (rc) return rc;
    VqGeom g;
    g.grid = v.dims;
    g.rz = ranges_host[0];
    g.ry = ranges_host[1];
    g.rx = ranges_host[2];
    g.nsample = nsample;
    g.radius2 = radius * radius;        // fp32, as the reference's kernel argument
    hipLaunchKernelGGL(voxel_query_kernel, dim3(cdiv(M, VQ_BLOCK)), dim3(VQ_BLOCK), 0, (hipStream_t)stream, new_xyz,
                       (const int4*)new_coords, M, xyz, N, (const uint2*)v.cells, (const int*)rowof, g, (int*)idx, empty);
    TODA_LAUNCH_CHECK();
    return TODA_OK;
}

extern "C" size_t toda_voxel_pool_moments_doubles(void) { return (size_t)VM_BLOCKS * 9 + 12; }

extern "C" int toda_voxel_pool_moments(const int32_t* idx, const uint8_t* empty, int M, int nsample, const float* xyz, int N,
                                       const float* new_xyz, double* ws, void* stream) {
    int rc = pool_check_sizes("voxel_pool_moments", M, nsample, VP_MAX_NSAMPLE, N, 1);
    if (rc) return rc;
    TODA_CHECK_ARG(M >= 1, "voxel_pool_moments: no grid points");
    TODA_CHECK_ARG(idx && empty && new_xyz && ws && (N == 0 || xyz), "voxel_pool_moments: null pointer");
    hipStream_t s = (hipStream_t)stream;
    double* part = ws + 12;
    hipLaunchKernelGGL(voxel_pool_moments_kernel, dim3(VM_BLOCKS), dim3(VP_BLOCK), 0, s, (const int*)idx, empty, M, nsample, xyz, N,
                       new_xyz, part);
    hipLaunchKernelGGL(voxel_pool_moments_fold_kernel, dim3(1), dim3(64), 0, s, (const double*)part, VM_BLOCKS,
                       (long long)M * nsample, ws);
    TODA_LAUNCH_CHECK();
    return TODA_OK;
}

extern "C" int toda_voxel_pool_fwd(const float* f, int N, int C, const int32_t* idx, const uint8_t* empty, int M, int nsample,
                                   const float* xyz, const float* new_xyz, const float* ab, float* out, uint8_t* arg, void* stream) {
    int rc = pool_check_sizes("voxel_pool_fwd", M, nsample, VP_MAX_NSAMPLE, N, C);
    if (rc) return rc;
    if (M == 0) return TODA_OK;
    TODA_CHECK_ARG(idx && empty && new_xyz && ab && out && (N == 0 || (f && xyz)), "voxel_pool_fwd: null pointer");
    hipLaunchKernelGGL(voxel_pool_fwd_kernel, dim3(cdiv(M, VP_POINTS)), dim3(VP_BLOCK), 0, (hipStream_t)stream, f, N, C, (const int*)idx,
                       empty, M, nsample, xyz, new_xyz, (const float4*)ab, out, arg);
    TODA_LAUNCH_CHECK();
    return TODA_OK;
}

extern "C" size_t toda_voxel_pool_table_bytes(int M, int nsample, int N) {
    if (M < 0 || nsample < 1 || N < 0) return 0;
    return vt_layout(M, nsample, N).bytes + 256;
}

extern "C" int toda_voxel_pool_table(const int32_t* idx, const uint8_t* empty, int M, int nsample, int N, int32_t* off, int32_t* ent,
                                     void* ws, size_t ws_bytes, void* stream) {
    // not bounded by VP_MAX_NSAMPLE: the SA gather (nsample <= 254) and the BEV taps (4) build their tables here too
    TODA_CHECK_ARG(M >= 0 && N >= 0 && nsample >= 1 && (long long)M * nsample < (1LL << 31), "voxel_pool_table: M=%d nsample=%d N=%d",
                   M, nsample, N);
    TODA_CHECK_ARG(off && ws && (M == 0 || (idx && empty && ent)), "voxel_pool_table: null pointer");
    const VtLayout L = vt_layout(M, nsample, N);
    if (ws_bytes < L.bytes) {
        set_error("voxel_pool_table: workspace of %zu bytes, need %zu", ws_bytes, L.bytes);
        return TODA_EWORKSPACE;
    }
    hipStream_t s = (hipStream_t)stream;
    char* w = (char*)ws;
    const int E = M * nsample;
    TODA_HIP(hipMemsetAsync(off, 0, (size_t)(N + 1) * 4, s));
    if (E == 0) return TODA_OK;
    hipLaunchKernelGGL(voxel_pool_keys_kernel, dim3(cdiv(E, VP_BLOCK)), dim3(VP_BLOCK), 0, s, (const int*)idx, empty, M, nsample, N,
                       (int32_t*)(w + L.sort.ka), (int32_t*)(w + L.sort.va), off);
    TODA_LAUNCH_CHECK();
    int rc = exclusive_scan(PlainAccess{off}, (long long)N + 1, (int32_t*)(w + L.scan_part), nullptr, s);
    if (rc) return rc;
    const int32_t* sval;
    rc = radix_sort_pairs(w, L.sort, E, (long long)N + 1, nullptr, &sval, s);          // keys run to N (the empty-ball key)
    if (rc) return rc;
    TODA_HIP(hipMemcpyAsync(ent, sval, (size_t)E * 4, hipMemcpyDeviceToDevice, s));
    return TODA_OK;
}

extern "C" int toda_voxel_pool_bwd_feat(const float* gout, const uint8_t* arg, int M, int nsample, int C, const int32_t* off,
                                        const int32_t* ent, int N, float* gf, void* stream) {
    int rc = pool_check_sizes("voxel_pool_bwd_feat", M, nsample, VP_MAX_NSAMPLE, N, C);
    if (rc) return rc;
    if (N == 0) return TODA_OK;
    TODA_CHECK_ARG(off && gf && (M == 0 || (gout && arg && ent)), "voxel_pool_bwd_feat: null pointer");
    hipLaunchKernelGGL(voxel_pool_bwd_feat_kernel, dim3(cdiv((long long)N * C, VP_BLOCK)), dim3(VP_BLOCK), 0, (hipStream_t)stream, gout, arg,
                       nsample, C, off, ent, N, gf);
    TODA_LAUNCH_CHECK();
    return TODA_OK;
}

extern "C" size_t toda_voxel_pool_bwd_pos_doubles(int C) { return C < 1 ? 0 : (size_t)VB_BLOCKS * C * 4; }

extern "C" int toda_voxel_pool_bwd_pos(const float* gout, const uint8_t* arg, const int32_t* idx, const uint8_t* empty, int M, int nsample,
                                       int C, const float* xyz, int N, const float* new_xyz, double* ws, float* gab, void* stream) {
    int rc = pool_check_sizes("voxel_pool_bwd_pos", M, nsample, VP_MAX_NSAMPLE, N, C);
    if (rc) return rc;
    TODA_CHECK_ARG(ws && gab && (M == 0 || (gout && arg && idx && empty && new_xyz)) && (N == 0 || xyz), "voxel_pool_bwd_pos: null pointer");
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(voxel_pool_bwd_pos_kernel, dim3(VB_BLOCKS, cdiv(C, 64)), dim3(VP_BLOCK), 0, s, gout, arg, (const int*)idx, empty, M,
                       nsample, C, xyz, N, new_xyz, ws);
    hipLaunchKernelGGL(pool_fold_partials_kernel, dim3(cdiv(C * 4, FOLD_BLOCK)), dim3(FOLD_BLOCK), 0, s, (const double*)ws, VB_BLOCKS, C * 4, gab);
    TODA_LAUNCH_CHECK();
    return TODA_OK;
}
