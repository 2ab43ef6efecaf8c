// surfview_math.h -- the arithmetic of the surface view: parallel projection, front-face coverage, the order-free
// depth key, the three interpolation modes and the composition, in float64 with + - * / and sqrt in the stated order.  Plain C++
// without a GPU construct, like meshvis_math.h (whose edge function and pixel span it shares): the very text the kernels of
// k_surfview.hip run also compiles for the host (tests/surfview_host_emu.cpp).  Compile with -ffp-contract=off.
#pragma once
#include "meshvis_math.h"

namespace ivx_surfview {

using ivx_meshvis::edge_fn;
using ivx_meshvis::pixel_span;

constexpr uint64_t KEY_EMPTY = ~(uint64_t)0;

// float32 bits -> unsigned order: smaller float, smaller word (the sign bit decides, so -0 sorts just below +0)
IVX_HD inline uint32_t depth_ord(uint32_t bits) { return (bits & 0x80000000u) ? ~bits : (bits ^ 0x80000000u); }
IVX_HD inline uint32_t depth_bits(uint32_t ord) { return (ord & 0x80000000u) ? (ord ^ 0x80000000u) : ~ord; }

IVX_HD inline double dot3(double dx, double dy, double dz, const double *a) { return (dx * a[0] + dy * a[1]) + dz * a[2]; }

struct Tri {
    double x[3], y[3], t[3], area;
    uint32_t id[3];
    int x0, x1, y0, y1; // clamped pixel box, inclusive
};

IVX_HD inline bool finite3(const float *p) {
    return p[0] - p[0] == 0.0f && p[1] - p[1] == 0.0f && p[2] - p[2] == 0.0f; // (inf - inf and nan - nan are nan)
}

// the three corners on the screen; false for an id out of range, a repeated id or a corner that is not finite
IVX_HD inline bool project_tri(const ivx_surface_camera &C, const float *verts, int64_t nverts, const int32_t *faces, int64_t t,
                               Tri &T) {
    const double px = 2.0 * C.parallel_scale / (double)C.height;
#pragma unroll
    for (int q = 0; q < 3; q++) {
        T.id[q] = (uint32_t)faces[3 * t + q];
        if ((int64_t)T.id[q] >= nverts) return false;
        const float *p = verts + 3 * (int64_t)T.id[q];
        if (!finite3(p)) return false;
        const double dx = (double)p[0] - C.focal[0], dy = (double)p[1] - C.focal[1], dz = (double)p[2] - C.focal[2];
        T.x[q] = dot3(dx, dy, dz, C.right) / px + 0.5 * (double)C.width;
        T.y[q] = 0.5 * (double)C.height - dot3(dx, dy, dz, C.up) / px;
        T.t[q] = dot3(dx, dy, dz, C.dir);
    }
    if (T.id[0] == T.id[1] || T.id[1] == T.id[2] || T.id[0] == T.id[2]) return false;
    T.area = edge_fn(T.x[0], T.y[0], T.id[0], T.x[1], T.y[1], T.id[1], T.x[2], T.y[2]);
    return true;
}

// ... and its pixel box; false when the triangle draws nothing (back-facing, zero area, outside the viewport)
IVX_HD inline bool load_tri(const ivx_surface_camera &C, const float *verts, int64_t nverts, const int32_t *faces, int64_t t, Tri &T) {
    if (!project_tri(C, verts, nverts, faces, t, T)) return false;
    if (!(T.area < 0.0)) return false; // front faces only (rows grow downward)
    pixel_span(fmin(fmin(T.x[0], T.x[1]), T.x[2]), fmax(fmax(T.x[0], T.x[1]), T.x[2]), C.width, T.x0, T.x1);
    pixel_span(fmin(fmin(T.y[0], T.y[1]), T.y[2]), fmax(fmax(T.y[0], T.y[1]), T.y[2]), C.height, T.y0, T.y1);
    return T.x1 >= T.x0 && T.y1 >= T.y0;
}

struct Edges {
    double bc, ca, ab;
};
IVX_HD inline Edges edges_at(const Tri &T, int i, int j) {
    const double qx = (double)i + 0.5, qy = (double)j + 0.5;
    Edges e;
    e.ab = edge_fn(T.x[0], T.y[0], T.id[0], T.x[1], T.y[1], T.id[1], qx, qy);
    e.bc = edge_fn(T.x[1], T.y[1], T.id[1], T.x[2], T.y[2], T.id[2], qx, qy);
    e.ca = edge_fn(T.x[2], T.y[2], T.id[2], T.x[0], T.y[0], T.id[0], qx, qy);
    return e;
}

// key of front-facing triangle `tri` at the centre of pixel (i, j); false when the centre is not covered
IVX_HD inline bool pixel_key(const Tri &T, int i, int j, uint32_t tri, uint64_t &key) {
    const Edges e = edges_at(T, i, j);
    if (!(e.ab <= 0.0 && e.bc <= 0.0 && e.ca <= 0.0)) return false;
    const float t = (float)(((e.bc * T.t[0] + e.ca * T.t[1]) + e.ab * T.t[2]) / T.area);
    uint32_t bits;
    memcpy(&bits, &t, 4);
    key = ((uint64_t)depth_ord(bits) << 32) | tri;
    return true;
}

IVX_HD inline double headlight(double nx, double ny, double nz, const double *dir) {
    const double s = -((nx * dir[0] + ny * dir[1]) + nz * dir[2]);
    return s > 0.0 ? s : 0.0;
}
IVX_HD inline double headlight_unit(double nx, double ny, double nz, const double *dir) {
    const double len = sqrt((nx * nx + ny * ny) + nz * nz);
    if (!(len > 0.0)) return 0.0;
    return headlight(nx / len, ny / len, nz / len, dir);
}

// diffuse intensity of layer L's triangle `tri` at the centre of pixel (i, j); false when the key cannot be this layer's
IVX_HD inline bool shade(const ivx_surface_camera &C, const ivx_surface_layer &L, uint32_t tri, int i, int j, int mode, double &I) {
    Tri T;
    if ((int64_t)tri >= L.ntris || !project_tri(C, L.verts, L.nverts, L.faces, tri, T)) return false;
    if (mode == IVX_SURFACE_FLAT || !L.normals) {
        const float *a = L.verts + 3 * (int64_t)T.id[0], *b = L.verts + 3 * (int64_t)T.id[1], *c = L.verts + 3 * (int64_t)T.id[2];
        const double ux = (double)b[0] - (double)a[0], uy = (double)b[1] - (double)a[1], uz = (double)b[2] - (double)a[2];
        const double vx = (double)c[0] - (double)a[0], vy = (double)c[1] - (double)a[1], vz = (double)c[2] - (double)a[2];
        I = headlight_unit(uy * vz - uz * vy, uz * vx - ux * vz, ux * vy - uy * vx, C.dir);
        return true;
    }
    const Edges e = edges_at(T, i, j);
    const double la = e.bc / T.area, lb = e.ca / T.area, lc = e.ab / T.area;
    const float *na = L.normals + 3 * (int64_t)T.id[0], *nb = L.normals + 3 * (int64_t)T.id[1], *nc = L.normals + 3 * (int64_t)T.id[2];
    if (mode == IVX_SURFACE_GOURAUD) {
        const double ia = headlight((double)na[0], (double)na[1], (double)na[2], C.dir);
        const double ib = headlight((double)nb[0], (double)nb[1], (double)nb[2], C.dir);
        const double ic = headlight((double)nc[0], (double)nc[1], (double)nc[2], C.dir);
        I = (la * ia + lb * ib) + lc * ic;
        return true;
    }
    I = headlight_unit((la * (double)na[0] + lb * (double)nb[0]) + lc * (double)nc[0],
                       (la * (double)na[1] + lb * (double)nb[1]) + lc * (double)nc[1],
                       (la * (double)na[2] + lb * (double)nb[2]) + lc * (double)nc[2], C.dir);
    return true;
}

IVX_HD inline uint8_t to_u8(float v) {
    const double x = floor(255.0 * (double)v + 0.5);
    if (!(x > 0.0)) return 0; // (a number that is none included)
    return x > 255.0 ? (uint8_t)255 : (uint8_t)x;
}

// One pixel of the picture: the layers' fragments sorted by (ord depth, layer), everything behind the first opaque one
// dropped, the rest blended far to near over the background.  rgba[4]; id[2] = (layer, triangle) of the nearest fragment or
// -1; *t its depth or +inf.
IVX_HD inline void resolve_pixel(const ivx_surface_camera &C, const ivx_surface_layer *layers, int nlayers, int mode,
                                 const float *background, int i, int j, float *rgba, int32_t *id, float *t) {
    const int64_t pix = (int64_t)j * C.width + i;
    uint64_t sk[IVX_SURFACE_MAX_LAYERS]; // (ord depth << 32) | layer, all ones where the layer has nothing here
    uint32_t tri[IVX_SURFACE_MAX_LAYERS];
    uint64_t cut = KEY_EMPTY, nearest = KEY_EMPTY;
    uint32_t nearest_tri = 0;
#pragma unroll
    for (int k = 0; k < IVX_SURFACE_MAX_LAYERS; k++) {
        sk[k] = KEY_EMPTY;
        tri[k] = 0;
        if (k < nlayers) {
            const uint64_t key = layers[k].keys[pix];
            if (key != KEY_EMPTY) {
                sk[k] = (key & 0xffffffff00000000ull) | (uint64_t)k;
                tri[k] = (uint32_t)key;
                if (sk[k] < nearest) {
                    nearest = sk[k];
                    nearest_tri = tri[k];
                }
                if (layers[k].opacity == 1.0f && sk[k] < cut) cut = sk[k];
            }
        }
    }
    double c[3] = {(double)background[0], (double)background[1], (double)background[2]}, a = 0.0;
    uint64_t prev = KEY_EMPTY; // far to near: the largest sort key below the one before, not behind the cut
    for (int n = 0; n < IVX_SURFACE_MAX_LAYERS; n++) {
        uint64_t m = 0;
        uint32_t mt = 0;
        bool any = false;
#pragma unroll
        for (int k = 0; k < IVX_SURFACE_MAX_LAYERS; k++)
            if (sk[k] < prev && sk[k] <= cut && (!any || sk[k] > m)) {
                m = sk[k];
                mt = tri[k];
                any = true;
            }
        if (!any) break;
        prev = m;
        const ivx_surface_layer &L = layers[(int)(m & 7u)];
        double I;
        if (!shade(C, L, mt, i, j, mode, I)) continue;
        const double al = (double)L.opacity;
        if (L.opacity == 1.0f) {
            for (int q = 0; q < 3; q++) c[q] = (double)L.rgb[q] * I;
            a = 1.0;
        } else {
            for (int q = 0; q < 3; q++) c[q] = (al * (double)L.rgb[q]) * I + (1.0 - al) * c[q];
            a = al + (1.0 - al) * a;
        }
    }
    rgba[0] = (float)c[0];
    rgba[1] = (float)c[1];
    rgba[2] = (float)c[2];
    rgba[3] = (float)a;
    if (nearest == KEY_EMPTY) {
        id[0] = id[1] = -1;
        *t = INFINITY;
    } else {
        id[0] = (int32_t)(nearest & 7u);
        id[1] = (int32_t)nearest_tri;
        const uint32_t bits = depth_bits((uint32_t)(nearest >> 32));
        memcpy(t, &bits, 4);
    }
}

} // namespace ivx_surfview
