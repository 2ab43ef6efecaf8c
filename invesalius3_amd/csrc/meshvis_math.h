// meshvis_math.h -- the arithmetic of the surface visibility rules: projection, pixel box, edge functions, depth and
// the point test, in float64 with + - * / in the stated order.  Plain C++ without a GPU construct, so that the very text the
// kernels of k_meshvis.hip run can also be compiled for the host and compared with the numpy restatement where there is no GPU
// (tests/meshvis_host_emu.cpp, tests/test_meshvis_host.py).  Compile with -ffp-contract=off.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "../../include/ivx.h"

#if defined(__HIPCC__)
#define IVX_HD __host__ __device__
#else
#define IVX_HD
#endif

namespace ivx_meshvis {

constexpr uint32_t DEPTH_ONE = 0x3f800000u; // 1.0f

struct Proj {
    double xs, ys, zw;
    bool ok;
};

// the projection of ivx.h, in its stated order
IVX_HD inline Proj project(const ivx_mesh_view &V, const float *p) {
    const double dx = (double)p[0] - V.eye[0], dy = (double)p[1] - V.eye[1], dz = (double)p[2] - V.eye[2];
    const double xe = (dx * V.right[0] + dy * V.right[1]) + dz * V.right[2];
    const double ye = (dx * V.up[0] + dy * V.up[1]) + dz * V.up[2];
    const double ze = (dx * V.fwd[0] + dy * V.fwd[1]) + dz * V.fwd[2];
    Proj r;
    r.ok = ze > 0.0;
    r.xs = (xe / (ze * V.tan_half * V.aspect) + 1.0) * 0.5 * (double)V.width;
    r.ys = (ye / (ze * V.tan_half) + 1.0) * 0.5 * (double)V.height;
    r.zw = (V.zfar * (ze - V.znear)) / (ze * (V.zfar - V.znear));
    return r;
}

// edge function of a -> b at q, evaluated from the end point with the smaller vertex id
IVX_HD inline double edge_fn(double ax, double ay, uint32_t ia, double bx, double by, uint32_t ib, double qx,
                                          double qy) {
    if (ia < ib) return (bx - ax) * (qy - ay) - (by - ay) * (qx - ax);
    return -((ax - bx) * (qy - by) - (ay - by) * (qx - bx));
}

struct Tri {
    double x[3], y[3], z[3], area;
    uint32_t id[3];
    int x0, x1, y0, y1; // clamped pixel box, inclusive; empty when x1 < x0 or y1 < y0
};

// first / last pixel whose centre lies in [lo, hi], clamped to [0, n - 1] (clamped as doubles: the cast is always in range)
IVX_HD inline void pixel_span(double lo, double hi, int n, int &p0, int &p1) {
    p0 = (int)ceil(fmin(fmax(lo - 0.5, 0.0), (double)n));
    p1 = (int)floor(fmin(fmax(hi - 0.5, -1.0), (double)(n - 1)));
}

IVX_HD inline bool load_tri(const ivx_mesh_view &V, const float *verts, int64_t nverts,
                                         const int32_t *faces, int64_t t, Tri &T) {
    bool ok = true;
#pragma unroll
    for (int q = 0; q < 3; q++) {
        T.id[q] = (uint32_t)faces[3 * t + q];
        if ((int64_t)T.id[q] >= nverts) return false;
        const Proj p = project(V, verts + 3 * (int64_t)T.id[q]);
        ok = ok && p.ok;
        T.x[q] = p.xs;
        T.y[q] = p.ys;
        T.z[q] = p.zw;
    }
    if (!ok || T.id[0] == T.id[1] || T.id[1] == T.id[2] || T.id[0] == T.id[2]) return false;
    T.area = edge_fn(T.x[0], T.y[0], T.id[0], T.x[1], T.y[1], T.id[1], T.x[2], T.y[2]);
    if (!(T.area > 0.0 || T.area < 0.0)) return false; // zero area (or not a number): covers nothing
    pixel_span(fmin(fmin(T.x[0], T.x[1]), T.x[2]), fmax(fmax(T.x[0], T.x[1]), T.x[2]), V.width, T.x0, T.x1);
    pixel_span(fmin(fmin(T.y[0], T.y[1]), T.y[2]), fmax(fmax(T.y[0], T.y[1]), T.y[2]), V.height, T.y0, T.y1);
    return T.x1 >= T.x0 && T.y1 >= T.y0;
}

// depth bits of triangle T at the centre of pixel (i, j); false when the centre is not covered or the depth cannot win
IVX_HD inline bool pixel_depth_bits(const Tri &T, int i, int j, uint32_t &bits) {
    const double qx = (double)i + 0.5, qy = (double)j + 0.5;
    const double e_ab = edge_fn(T.x[0], T.y[0], T.id[0], T.x[1], T.y[1], T.id[1], qx, qy);
    const double e_bc = edge_fn(T.x[1], T.y[1], T.id[1], T.x[2], T.y[2], T.id[2], qx, qy);
    const double e_ca = edge_fn(T.x[2], T.y[2], T.id[2], T.x[0], T.y[0], T.id[0], qx, qy);
    const bool in = T.area > 0.0 ? (e_ab >= 0.0 && e_bc >= 0.0 && e_ca >= 0.0) : (e_ab <= 0.0 && e_bc <= 0.0 && e_ca <= 0.0);
    if (!in) return false;
    const float z = (float)(((e_bc * T.z[0] + e_ca * T.z[1]) + e_ab * T.z[2]) / T.area);
    memcpy(&bits, &z, 4);
    return bits < DEPTH_ONE; // 1.0 and beyond never wins, and a negative depth has no place in the unsigned order
}

// the point test of one view against its depth buffer
IVX_HD inline bool point_visible(const ivx_mesh_view &V, const float *p, const float *depth) {
    const Proj r = project(V, p);
    if (!r.ok || !(r.xs >= 0.0 && r.xs < (double)V.width && r.ys >= 0.0 && r.ys < (double)V.height)) return false;
    const int i = (int)r.xs, j = (int)r.ys;
    return r.zw < (double)depth[(int64_t)j * V.width + i] + 0.01;
}

} // namespace ivx_meshvis
