// scene3d_math.h -- the arithmetic the 3-D scene adds to the ray casters and the surface view: the hit of
// a pixel's ray on a slice plane, the plane's bilinear texture sample, the sample K_f a fragment goes before, and the choice of
// the nearest remaining fragment.  float64 with + - * / in the stated order, float32 where the rules say so.  Plain C++ without
// a GPU construct, like surfview_math.h: the very text k_scene3d.hip runs also compiles for the host
// (tests/scene3d_host_emu.cpp).  Compile with -ffp-contract=off.
#pragma once
#include "surfview_math.h"

namespace ivx_scene3d {

using ivx_surfview::KEY_EMPTY;
using ivx_surfview::depth_bits;
using ivx_surfview::depth_ord;

constexpr int MAX_FRAGS = IVX_SURFACE_MAX_LAYERS + IVX_SCENE_MAX_PLANES; // layers 0 .. 7 surfaces, 8 .. 10 planes
constexpr uint64_t LAYER_MASK = 15u;

// sort key of a fragment at float32 depth t on `layer`: (ord depth, layer index)
IVX_HD inline uint64_t frag_key(float t, int layer) {
    uint32_t bits;
    memcpy(&bits, &t, 4);
    return ((uint64_t)depth_ord(bits) << 32) | (uint64_t)layer;
}
IVX_HD inline float key_depth(uint64_t key) {
    const uint32_t bits = depth_bits((uint32_t)(key >> 32));
    float t;
    memcpy(&t, &bits, 4);
    return t;
}

// The ray P0 + t dir on the plane of `orientation` at image slice `slice`: false when the ray runs in the plane or leaves the
// rectangle of the w x h voxel centres.  `off` is 1 when P0 counts positions on the padded mask matrix (origin moved by one
// spacing, index = image index + 1), else 0.  t: the float32 depth; (u, v): the index position along the picture's columns / rows.
IVX_HD inline bool plane_hit(const double *P0, const double *dir, const double *spacing, int orientation, int slice, int h, int w,
                             int off, float &t, float &u, float &v) {
    const int a = orientation == IVX_SCENE_AXIAL ? 2 : (orientation == IVX_SCENE_CORONAL ? 1 : 0);
    if (dir[a] == 0.0) return false;
    const double n = (double)(slice + off);
    const double c = a == 1 ? -(n * spacing[1]) : n * spacing[a];
    const double tp = (c - P0[a]) / dir[a];
    const double qx = P0[0] + tp * dir[0], qy = P0[1] + tp * dir[1], qz = P0[2] + tp * dir[2];
    const double ix = qx / spacing[0] - (double)off, iy = -qy / spacing[1] - (double)off, iz = qz / spacing[2] - (double)off;
    const double du = a == 0 ? iy : ix, dv = a == 2 ? iy : iz;
    if (!(0.0 <= du && du <= (double)(w - 1) && 0.0 <= dv && dv <= (double)(h - 1))) return false;
    t = (float)tp;
    u = (float)du;
    v = (float)dv;
    return true;
}

IVX_HD inline float lerp32(float a, float b, float f) { return a + f * (b - a); }

// the RGB8 picture (h rows x w columns, dense) at column position u, row position v: bilinear in float32 with the index
// clamping of the ray casters' trilinear sample, along the columns first; then / 255
IVX_HD inline void plane_texel(const uint8_t *pic, int h, int w, float u, float v, float *rgb) {
    int i0 = (int)u, j0 = (int)v;
    i0 = i0 < (w - 2 > 0 ? w - 2 : 0) ? i0 : (w - 2 > 0 ? w - 2 : 0);
    j0 = j0 < (h - 2 > 0 ? h - 2 : 0) ? j0 : (h - 2 > 0 ? h - 2 : 0);
    const int i1 = i0 + 1 < w - 1 ? i0 + 1 : w - 1, j1 = j0 + 1 < h - 1 ? j0 + 1 : h - 1;
    const float fu = u - (float)i0, fv = v - (float)j0;
    const uint8_t *r0 = pic + (int64_t)j0 * w * 3, *r1 = pic + (int64_t)j1 * w * 3;
#pragma unroll
    for (int q = 0; q < 3; q++) {
        const float top = lerp32((float)r0[3 * i0 + q], (float)r0[3 * i1 + q], fu);
        const float bot = lerp32((float)r1[3 * i0 + q], (float)r1[3 * i1 + q], fu);
        rgb[q] = lerp32(top, bot, fv) / 255.0f;
    }
}

// the sample a fragment at depth t goes before: clamp(ceil((t - tin) / dt), 0, kmax + 1)
IVX_HD inline long long frag_sample(float t, double tin, double dt, long long kmax) {
    const double k = ceil(((double)t - tin) / dt);
    if (!(k > 0.0)) return 0;
    if (k > (double)(kmax + 1)) return kmax + 1;
    return (long long)k;
}

// The nearest remaining fragment of sk[0 .. MAX_FRAGS): the smallest key that is not empty and, unless `first`, above `prev`
// (keys differ in their layer bits).  Fully unrolled over constant indices, so the keys stay in registers.
IVX_HD inline bool next_fragment(const uint64_t *sk, bool first, uint64_t prev, uint64_t &m) {
    bool any = false;
    m = KEY_EMPTY;
#pragma unroll
    for (int k = 0; k < MAX_FRAGS; k++)
        if (sk[k] != KEY_EMPTY && (first || sk[k] > prev) && sk[k] < m) {
            m = sk[k];
            any = true;
        }
    return any;
}

} // namespace ivx_scene3d
