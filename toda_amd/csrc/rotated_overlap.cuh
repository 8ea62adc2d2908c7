// Rotated-rectangle overlap shared by nms.hip (BEV IoU matrix, NMS) and roi_head.hip (3-D IoU max per roi): the
// intersection polygon of two (x, y, z, dx, dy, dz, heading) boxes in BEV, as in the reference's
// pcdet/ops/iou3d_nms/src/iou3d_nms_kernel.cu.  Header-only: every translation unit gets its own inlined copy.
#pragma once
#include <hip/hip_runtime.h>

namespace toda {

struct P2 {
    float x, y;
};

__device__ __forceinline__ float cross3(P2 p1, P2 p2, P2 p0) {
    return (p1.x - p0.x) * (p2.y - p0.y) - (p2.x - p0.x) * (p1.y - p0.y);
}

// proper crossing of segments p0p1 and q0q1 (touching end points do not count)
__device__ __forceinline__ bool seg_cross(P2 p1, P2 p0, P2 q1, P2 q0, P2* hit) {
    const bool boxes_meet = fminf(p0.x, p1.x) <= fmaxf(q0.x, q1.x) && fminf(q0.x, q1.x) <= fmaxf(p0.x, p1.x) &&
                            fminf(p0.y, p1.y) <= fmaxf(q0.y, q1.y) && fminf(q0.y, q1.y) <= fmaxf(p0.y, p1.y);
    if (!boxes_meet) return false;
    const float s1 = cross3(q0, p1, p0), s2 = cross3(p1, q1, p0), s3 = cross3(p0, q1, q0), s4 = cross3(q1, p1, q0);
    if (!(s1 * s2 > 0.f && s3 * s4 > 0.f)) return false;
    const float s5 = cross3(q1, p1, p0);
    if (fabsf(s5 - s1) > 1e-8f) {
        hit->x = (s5 * q0.x - s1 * q1.x) / (s5 - s1);
        hit->y = (s5 * q0.y - s1 * q1.y) / (s5 - s1);
    } else {
        const float a0 = p0.y - p1.y, b0 = p1.x - p0.x, c0 = p0.x * p1.y - p1.x * p0.y;
        const float a1 = q0.y - q1.y, b1 = q1.x - q0.x, c1 = q0.x * q1.y - q1.x * q0.y;
        const float D = a0 * b1 - a1 * b0;
        hit->x = (b0 * c1 - b1 * c0) / D;
        hit->y = (a1 * c0 - a0 * c1) / D;
    }
    return true;
}

__device__ __forceinline__ bool inside(const float* box, P2 p) {  // 1e-2 margin as in the reference
    const float c = cosf(-box[6]), s = sinf(-box[6]);
    const float rx = (p.x - box[0]) * c + (p.y - box[1]) * (-s);
    const float ry = (p.x - box[0]) * s + (p.y - box[1]) * c;
    return fabsf(rx) < box[3] / 2 + 1e-2f && fabsf(ry) < box[4] / 2 + 1e-2f;
}

__device__ __forceinline__ void corners(const float* b, P2* c) {
    const float hx = b[3] / 2, hy = b[4] / 2, cs = cosf(b[6]), sn = sinf(b[6]);
    const float lx[4] = {-hx, hx, hx, -hx}, ly[4] = {-hy, -hy, hy, hy};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float px = b[0] + lx[k], py = b[1] + ly[k];
        c[k].x = (px - b[0]) * cs + (py - b[1]) * (-sn) + b[0];
        c[k].y = (px - b[0]) * sn + (py - b[1]) * cs + b[1];
    }
    c[4] = c[0];
}

// area of the intersection of two rotated rectangles (x, y, z, dx, dy, dz, heading)
__device__ inline float overlap_area(const float* a, const float* b) {
    P2 ca[5], cb[5], pts[16], ctr = {0.f, 0.f};
    int cnt = 0;
    corners(a, ca);
    corners(b, cb);
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j)
            if (seg_cross(ca[i + 1], ca[i], cb[j + 1], cb[j], &pts[cnt])) {
                ctr.x += pts[cnt].x;
                ctr.y += pts[cnt].y;
                ++cnt;
            }
    for (int k = 0; k < 4; ++k) {
        if (inside(a, cb[k])) {
            ctr.x += cb[k].x;
            ctr.y += cb[k].y;
            pts[cnt++] = cb[k];
        }
        if (inside(b, ca[k])) {
            ctr.x += ca[k].x;
            ctr.y += ca[k].y;
            pts[cnt++] = ca[k];
        }
    }
    if (cnt == 0) return 0.f;
    ctr.x /= cnt;
    ctr.y /= cnt;
    float ang[16];
    for (int i = 0; i < cnt; ++i) ang[i] = atan2f(pts[i].y - ctr.y, pts[i].x - ctr.x);
    for (int j = 0; j < cnt - 1; ++j)  // <= 16 points: exchange sort by polar angle
        for (int i = 0; i < cnt - j - 1; ++i)
            if (ang[i] > ang[i + 1]) {
                const P2 t = pts[i];
                pts[i] = pts[i + 1];
                pts[i + 1] = t;
                const float ta = ang[i];
                ang[i] = ang[i + 1];
                ang[i + 1] = ta;
            }
    float area = 0.f;
    for (int k = 0; k < cnt - 1; ++k)
        area += (pts[k].x - pts[0].x) * (pts[k + 1].y - pts[0].y) - (pts[k].y - pts[0].y) * (pts[k + 1].x - pts[0].x);
    return fabsf(area) / 2.0f;
}

__device__ __forceinline__ float iou_bev(const float* a, const float* b) {
    const float sa = a[3] * a[4], sb = b[3] * b[4], so = overlap_area(a, b);
    return so / fmaxf(sa + sb - so, 1e-8f);
}

}  // namespace toda
