// What the point-table kernels of points.hip and points_local.hip share: the block size and the point-in-box tests.
#pragma once
#include "common.h"

namespace toda {

constexpr int PT_BLOCK = 256;

struct BoxPre {
    float cx, cy, cz, dx, dy, dz, cosa, sina;
};

// mode 0: roiaware_pool3d.cpp:121-141 (|z-cz| > dz/2 rejects, |local| < d/2 + 1e-2, fp64 compare)
// mode 1: augmentor_utils.py:474-491   (|z-cz| <= dz/2, |local| <= fp32(d/2 + 0.1))
// mode 2: roiaware_pool3d_kernel.cu:23-36 (as mode 0 with margin 1e-5 and fp32 cos / sin) - points_in_boxes_gpu
template <int MODE>
__device__ __forceinline__ bool point_in_box(float x, float y, float z, const BoxPre& b) {
    const float sz = z - b.cz;
    if (MODE == 0 || MODE == 2) {
        if ((double)fabsf(sz) > (double)b.dz / 2.0) return false;
    } else {
        if (!(fabsf(sz) <= b.dz / 2.0f)) return false;
    }
    const float sx = x - b.cx, sy = y - b.cy;
    const float lx = sx * b.cosa + sy * (-b.sina);
    const float ly = sx * b.sina + sy * b.cosa;
    if (MODE == 0 || MODE == 2) {
        const double m = MODE == 0 ? (double)1e-2f : (double)1e-5f;
        return fabs((double)lx) < (double)b.dx / 2.0 + m && fabs((double)ly) < (double)b.dy / 2.0 + m;
    }
    const float mx = b.dx / 2.0f + 0.1f, my = b.dy / 2.0f + 0.1f;
    return fabsf(lx) <= mx && fabsf(ly) <= my;
}

}  // namespace toda
