// Camera field-of-view test of a KITTI frame for gfx950: the one per-frame point pass of the reference's KittiDataset
// (kitti_dataset.py get_fov_flag, calibration_kitti.py lidar_to_rect / rect_to_img) that the point-table family of points.hip
// did not have.  A functor of points_common.cuh's pt_rows_kernel: one thread per point, no LDS, no atomics, 4*c bytes in and
// 4 bytes of flag out per point, so the kernel is bound by HBM traffic; the flags feed the stable compaction of points.hip
// (toda_rows_select_append).
//
// Arithmetic is fp32 in the reference's order of operations (-ffp-contract=off, no fused multiply-adds):
//   rect  = [x y z 1] . M        M = fp32(V2C^T . R0^T), 4 x 3, formed on the host
//   hom   = [rect 1] . P2^T      u = hom0 / rect_z, v = hom1 / rect_z, depth = hom2 - P2[2][3]
// numpy's matrix product may sum the four terms in another order, so a point within a few ulp of an image edge can differ.
// rect_z == 0 gives +-inf or NaN pixels; every comparison with them is false, as in numpy, and the flag is 0.
#include "common.h"
#include "points_common.cuh"

namespace toda {

struct FovCalib {
    float m[12];      // [4][3], row k = coefficient of x, y, z, 1
    float p2[12];     // [3][4]
    int img_h, img_w;
};

// functor of pt_rows_kernel (points_common.cuh)
template <bool VEC4>
struct FovFlags {
    FovCalib k;
    int32_t* __restrict__ flags;
    __device__ void operator()(int j, const float* __restrict__ p) const {
        float x, y, z;
        if (VEC4) {                     // c == 4 and a 16-byte aligned base: one 16-byte load per row
            const float4 q = *reinterpret_cast<const float4*>(p);
            x = q.x, y = q.y, z = q.z;
        } else {
            x = p[0], y = p[1], z = p[2];
        }
        const float rx = x * k.m[0] + y * k.m[3] + z * k.m[6] + k.m[9];
        const float ry = x * k.m[1] + y * k.m[4] + z * k.m[7] + k.m[10];
        const float rz = x * k.m[2] + y * k.m[5] + z * k.m[8] + k.m[11];
        const float h0 = rx * k.p2[0] + ry * k.p2[1] + rz * k.p2[2] + k.p2[3];
        const float h1 = rx * k.p2[4] + ry * k.p2[5] + rz * k.p2[6] + k.p2[7];
        const float h2 = rx * k.p2[8] + ry * k.p2[9] + rz * k.p2[10] + k.p2[11];
        const float u = h0 / rz, v = h1 / rz, depth = h2 - k.p2[11];
        // the image size is compared as numpy compares an fp32 column with an int32 scalar: in fp64
        const bool in = (u >= 0.f) & ((double)u < (double)k.img_w) & (v >= 0.f) & ((double)v < (double)k.img_h) & (depth >= 0.f);
        flags[j] = in ? 1 : 0;
    }
};

}  // namespace toda

using namespace toda;

extern "C" int toda_points_fov_flags(const float* points, int n, const int32_t* n_dev, int c, const float* m_host,
                                     const float* p2_host, int img_h, int img_w, int32_t* flags, void* stream) {
    PT_CHECK_SIZES("points_fov_flags");
    TODA_CHECK_ARG(img_h > 0 && img_w > 0, "points_fov_flags: image size %d x %d is not positive", img_h, img_w);
    PT_CHECK_TABLES(m_host && p2_host, "points_fov_flags: null calibration matrix");
    TODA_CHECK_ARG(points && flags, "points_fov_flags: null points or flags");
    FovCalib k;
    for (int i = 0; i < 12; ++i) k.m[i] = m_host[i], k.p2[i] = p2_host[i];
    k.img_h = img_h, k.img_w = img_w;
    if (c == 4 && ((uintptr_t)points & 15) == 0) return pt_rows_pass("points_fov_flags", points, n, n_dev, c, flags, FovFlags<true>{k, flags}, stream);
    return pt_rows_pass("points_fov_flags", points, n, n_dev, c, flags, FovFlags<false>{k, flags}, stream);
}
