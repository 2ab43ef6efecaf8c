// volren_ray.h -- what the two ray casters (k_volren.hip: the image through a preset; k_maskren.hip: the mask preview)
// share: the macro-cell and tile sizes, a pixel's parallel ray in index space with its sample range, the sample
// positions t_in + k dt (from k, never accumulated), and the landing sample of an empty-space jump.
#pragma once
#include "ivx_internal.h"

namespace {

constexpr int CELL = IVX_VOLREN_CELL;
constexpr int TILE = 8;                        // render tile edge: 64 rays = one wave
constexpr float OPAQUE = 1.0f - 1.0f / 4096.0f; // early ray termination

struct Dims {
    int nz, ny, nx;
};

__device__ __forceinline__ float lerpf(float a, float b, float f) { return a + f * (b - a); }

__device__ __forceinline__ float clampf(float v, float lo, float hi) { return fminf(fmaxf(v, lo), hi); }

__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}

struct RayCtx {
    float I0[3], S[3]; // index position of sample 0 and step per sample
    long long kmax;    // last sample index (-1: no sample)
    double tin;        // world distance of sample 0 from the pixel's plane
};

// the ray of pixel (px, py) in index space and its samples' range; false = the ray misses
__device__ bool setup_ray(const ivx_volren_params &p, const Dims &d, int px, int py, RayCtx &r) {
    double P0[3], A[3], B[3];
    for (int a = 0; a < 3; a++) P0[a] = p.origin[a] + (double)px * p.du[a] + (double)py * p.dv[a];
    A[0] = P0[0] / p.spacing[0];
    A[1] = -P0[1] / p.spacing[1];
    A[2] = P0[2] / p.spacing[2];
    B[0] = p.dir[0] / p.spacing[0];
    B[1] = -p.dir[1] / p.spacing[1];
    B[2] = p.dir[2] / p.spacing[2];
    const double hi[3] = {(double)(d.nx - 1), (double)(d.ny - 1), (double)(d.nz - 1)};
    double tin = -1e300, tout = 1e300;
    for (int a = 0; a < 3; a++) {
        if (B[a] != 0.0) {
            double t0 = (0.0 - A[a]) / B[a], t1 = (hi[a] - A[a]) / B[a];
            if (t0 > t1) {
                const double t = t0;
                t0 = t1;
                t1 = t;
            }
            tin = fmax(tin, t0);
            tout = fmin(tout, t1);
        } else if (A[a] < 0.0 || A[a] > hi[a]) {
            return false;
        }
    }
    if (p.clip) {
        double nd = 0.0, c0 = 0.0;
        for (int a = 0; a < 3; a++) {
            nd += p.clip_normal[a] * p.dir[a];
            c0 += p.clip_normal[a] * (P0[a] - p.clip_origin[a]);
        }
        if (nd > 0.0) tin = fmax(tin, -c0 / nd);
        else if (nd < 0.0) tout = fmin(tout, -c0 / nd);
        else if (c0 < 0.0) return false;
    }
    if (!(tin <= tout)) return false;
    r.kmax = (long long)floor((tout - tin) / p.dt);
    r.tin = tin;
    for (int a = 0; a < 3; a++) {
        r.I0[a] = (float)(A[a] + tin * B[a]);
        r.S[a] = (float)(B[a] * p.dt);
    }
    return true;
}

__device__ __forceinline__ void sample_pos(const RayCtx &r, const Dims &d, long long k, float &x, float &y, float &z) {
    const float fk = (float)k;
    x = clampf(r.I0[0] + fk * r.S[0], 0.0f, (float)(d.nx - 1));
    y = clampf(r.I0[1] + fk * r.S[1], 0.0f, (float)(d.ny - 1));
    z = clampf(r.I0[2] + fk * r.S[2], 0.0f, (float)(d.nz - 1));
}

// Samples k + 1 .. (returned) - 1 lie in the same macro cell as sample k (cell index (cx, cy, cz)): the landing sample
// is the first one at or past the cell's exit plane, accepted only if the sample before it is still in the cell (the
// positions are monotone in k along every axis, so then every sample in between is too); else k + 1.
__device__ __forceinline__ long long cell_exit(const RayCtx &r, const Dims &d, long long k, int cx, int cy, int cz) {
    const int c[3] = {cx, cy, cz};
    float kk = 3.0e38f;
    for (int a = 0; a < 3; a++) {
        if (r.S[a] > 0.0f) kk = fminf(kk, ((float)((c[a] + 1) * CELL) - r.I0[a]) / r.S[a]);
        else if (r.S[a] < 0.0f) kk = fminf(kk, ((float)(c[a] * CELL) - r.I0[a]) / r.S[a]);
    }
    if (!(kk < 9.0e18f)) return r.kmax + 1;
    long long kn = (long long)floorf(kk);
    if (kn <= k + 1) return k + 1;
    float x, y, z;
    sample_pos(r, d, kn - 1, x, y, z);
    if ((int)x / CELL != cx || (int)y / CELL != cy || (int)z / CELL != cz) return k + 1;
    return kn;
}

// -- host side: argument checks both renderers share
int check_shape(const int64_t shape[3], Dims &d) {
    IVX_REQUIRE(shape, IVX_EINVAL, "volren: null shape");
    for (int a = 0; a < 3; a++)
        IVX_REQUIRE(shape[a] >= 1 && shape[a] <= 32768, IVX_EINVAL, "volren: shape[%d] = %lld", a, (long long)shape[a]);
    d.nz = (int)shape[0];
    d.ny = (int)shape[1];
    d.nx = (int)shape[2];
    return IVX_OK;
}

Dims cell_dims(const Dims &d) {
    return Dims{(int)ivx::cdiv(d.nz, CELL), (int)ivx::cdiv(d.ny, CELL), (int)ivx::cdiv(d.nx, CELL)};
}

int check_params(const ivx_volren_params *p) {
    IVX_REQUIRE(p, IVX_EINVAL, "volren: null params");
    IVX_REQUIRE(p->width >= 1 && p->height >= 1 && p->width <= 32768 && p->height <= 32768, IVX_EINVAL,
                "volren: viewport %d x %d", p->width, p->height);
    IVX_REQUIRE(p->n_table >= 2 && p->n_table <= 65537, IVX_EINVAL, "volren: n_table %d (2 .. 65537)", p->n_table);
    IVX_REQUIRE(p->dt > 0.0 && p->spacing[0] > 0.0 && p->spacing[1] > 0.0 && p->spacing[2] > 0.0, IVX_EINVAL,
                "volren: sample distance and spacing must be positive");
    const double dn = p->dir[0] * p->dir[0] + p->dir[1] * p->dir[1] + p->dir[2] * p->dir[2];
    IVX_REQUIRE(dn > 0.5 && dn < 2.0, IVX_EINVAL, "volren: ray direction must be a unit vector");
    return IVX_OK;
}

} // namespace
