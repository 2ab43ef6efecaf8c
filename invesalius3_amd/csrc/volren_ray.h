// volren_ray.h -- the ray-casting core of the two renderers (k_volren.hip: the image through a preset; k_maskren.hip: the
// mask preview): the macro-cell and tile sizes, a pixel's parallel ray in index space with its sample range, the sample
// positions t_in + k dt (from k, never accumulated), the landing sample of an empty-space jump, and, templated on the
// field read (the dense uint16 image, the strided uint8 mask with its virtual apron), the macro-cell kernel, the
// trilinear sample, the headlight, the front-to-back composite loop, the pixel write and the sample counters
// (DESIGN.md 7d).  The MIP loop stays in k_volren.hip, the iso loop in k_maskren.hip.
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

// -- the fields: raw(z, y, x) reads the array, fetch(z, y, x) the logical field; with `apron` 1 logical index 0 of
// every axis is a virtual plane of `av`; transparent(): the composite loop may jump a cell with these (min, max)
struct DenseField { // the prepared uint16 image
    typedef uint16_t cell_t;
    static constexpr int apron = 0;
    static constexpr unsigned av = 0;
    const uint16_t *__restrict__ base;
    int64_t sz, sy; // slice and row pitch in voxels
    __device__ __forceinline__ unsigned raw(int z, int y, int x) const { return base[z * sz + y * sy + x]; }
    __device__ __forceinline__ float fetch(int z, int y, int x) const { return (float)raw(z, y, x); }
    // the table entries [min - 1, max + 1]: a sample between two voxels interpolates the entries around both
    __device__ __forceinline__ static bool transparent(const uint32_t *__restrict__ prefix, int nt, int mn, int mx) {
        return prefix[min(mx + 1, nt - 1) + 1] == prefix[max(mn - 1, 0)];
    }
};

struct Field { // the uint8 mask: byte strides, and with `apron` 1 array index = logical index - 1
    typedef uint8_t cell_t;
    const uint8_t *base;
    int64_t sz, sy, sx; // byte strides of the array
    int apron;
    unsigned av;
    __device__ __forceinline__ unsigned raw(int z, int y, int x) const { return base[z * sz + y * sy + x * sx]; }
    __device__ __forceinline__ float fetch(int z, int y, int x) const {
        if (apron) {
            if (z == 0 || y == 0 || x == 0) return (float)av;
            z--, y--, x--;
        }
        return (float)raw(z, y, x);
    }
    // the table entries [min, max]: a byte field sampled at an integer s has fraction 0, so entry floor(s) + 1 weighs
    // nothing at s == max
    __device__ __forceinline__ static bool transparent(const uint32_t *__restrict__ prefix, int, int mn, int mx) {
        return prefix[mx + 1] == prefix[mn];
    }
};

// min / max per macro cell with one voxel of apron on every side, cells cz0 .. of the logical field d: a thread per cell
template <class F>
__global__ __launch_bounds__(256) void k_cells(F v, Dims d, Dims c, int cz0, int64_t ncell,
                                              typename F::cell_t *__restrict__ cells) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= ncell) return;
    const int64_t ci = i + (int64_t)cz0 * c.ny * c.nx;
    const int cx = (int)(ci % c.nx), cy = (int)((ci / c.nx) % c.ny), cz = (int)(ci / ((int64_t)c.nx * c.ny));
    const int x0 = max(cx * CELL - 1, 0), x1 = min(cx * CELL + CELL, d.nx - 1);
    const int y0 = max(cy * CELL - 1, 0), y1 = min(cy * CELL + CELL, d.ny - 1);
    const int z0 = max(cz * CELL - 1, 0), z1 = min(cz * CELL + CELL, d.nz - 1);
    unsigned lo = (typename F::cell_t)~0u, hi = 0;
    const int a = v.apron;
    if (a && (x0 == 0 || y0 == 0 || z0 == 0)) lo = hi = v.av;
    for (int z = max(z0, a); z <= z1; z++)
        for (int y = max(y0, a); y <= y1; y++)
            for (int x = max(x0, a); x <= x1; x++) {
                const unsigned s = v.raw(z - a, y - a, x - a);
                lo = min(lo, s);
                hi = max(hi, s);
            }
    cells[2 * ci] = (typename F::cell_t)lo;
    cells[2 * ci + 1] = (typename F::cell_t)hi;
}

// trilinear interpolation at the logical index position (x, y, z), already clamped to the field
template <class F>
__device__ __forceinline__ float tri(const F &v, const Dims &d, float x, float y, float z) {
    int x0 = (int)x, y0 = (int)y, z0 = (int)z;
    x0 = min(x0, max(d.nx - 2, 0));
    y0 = min(y0, max(d.ny - 2, 0));
    z0 = min(z0, max(d.nz - 2, 0));
    const float fx = x - (float)x0, fy = y - (float)y0, fz = z - (float)z0;
    const int x1 = min(x0 + 1, d.nx - 1), y1 = min(y0 + 1, d.ny - 1), z1 = min(z0 + 1, d.nz - 1);
    const float c00 = lerpf(v.fetch(z0, y0, x0), v.fetch(z0, y0, x1), fx);
    const float c01 = lerpf(v.fetch(z0, y1, x0), v.fetch(z0, y1, x1), fx);
    const float c10 = lerpf(v.fetch(z1, y0, x0), v.fetch(z1, y0, x1), fx);
    const float c11 = lerpf(v.fetch(z1, y1, x0), v.fetch(z1, y1, x1), fx);
    return lerpf(lerpf(c00, c01, fy), lerpf(c10, c11, fy), fz);
}

struct Light {
    float ka, kd, ks, pw, dx, dy, dz, isx, isy, isz, hx, hy, hz;
};

__device__ __forceinline__ Light make_light(const ivx_volren_params &p, const Dims &d) {
    Light l;
    l.ka = (float)p.ambient, l.kd = (float)p.diffuse, l.ks = (float)p.specular, l.pw = (float)p.specular_power;
    l.dx = (float)p.dir[0], l.dy = (float)p.dir[1], l.dz = (float)p.dir[2];
    l.isx = (float)(0.5 / p.spacing[0]), l.isy = (float)(0.5 / p.spacing[1]), l.isz = (float)(0.5 / p.spacing[2]);
    l.hx = (float)(d.nx - 1), l.hy = (float)(d.ny - 1), l.hz = (float)(d.nz - 1);
    return l;
}

// the headlight of DESIGN.md section 7d at (x, y, z) on colour (cr, cg, cb)
template <class F>
__device__ __forceinline__ void shade_at(const F &v, const Dims &d, const Light &l, float x, float y, float z, float &cr,
                                         float &cg, float &cb) {
    // gradient in world axes: world y = -index y
    const float gx = (tri(v, d, fminf(x + 1.0f, l.hx), y, z) - tri(v, d, fmaxf(x - 1.0f, 0.0f), y, z)) * l.isx;
    const float gy = (tri(v, d, x, fmaxf(y - 1.0f, 0.0f), z) - tri(v, d, x, fminf(y + 1.0f, l.hy), z)) * l.isy;
    const float gz = (tri(v, d, x, y, fminf(z + 1.0f, l.hz)) - tri(v, d, x, y, fmaxf(z - 1.0f, 0.0f))) * l.isz;
    const float gn = sqrtf(gx * gx + gy * gy + gz * gz);
    float ndl = 0.0f;
    if (gn > 0.0f) ndl = fabsf(gx * l.dx + gy * l.dy + gz * l.dz) / gn;
    const float diff = l.ka + l.kd * ndl;
    const float spec = ndl > 0.0f ? l.ks * powf(ndl, l.pw) : 0.0f;
    cr = clampf(cr * diff + spec, 0.0f, 1.0f);
    cg = clampf(cg * diff + spec, 0.0f, 1.0f);
    cb = clampf(cb * diff + spec, 0.0f, 1.0f);
}

// Front-to-back compositing of the ray's samples over the background already in (r, g, b): classification by linear
// interpolation of the table, the headlight with p.shade, early termination at A >= OPAQUE, and with p.skip a jump over
// every cell that F::transparent() passes.
template <class F>
__device__ __forceinline__ void composite_ray(const F &v, const typename F::cell_t *__restrict__ cells, const Dims &d,
                                              const Dims &c, const float4 *__restrict__ table,
                                              const uint32_t *__restrict__ prefix, const ivx_volren_params &p,
                                              const RayCtx &ray, float &r, float &g, float &b, float &A,
                                              unsigned long long &n_taken, unsigned long long &n_skipped,
                                              unsigned long long &n_early) {
    const int nt = p.n_table;
    const Light l = make_light(p, d);
    float ar = 0.0f, ag = 0.0f, ab = 0.0f;
    for (long long k = 0; k <= ray.kmax;) {
        float x, y, z;
        sample_pos(ray, d, k, x, y, z);
        if (p.skip) {
            const int cx = (int)x / CELL, cy = (int)y / CELL, cz = (int)z / CELL;
            const int64_t ci = ((int64_t)cz * c.ny + cy) * c.nx + cx;
            if (F::transparent(prefix, nt, (int)cells[2 * ci], (int)cells[2 * ci + 1])) {
                const long long kn = cell_exit(ray, d, k, cx, cy, cz);
                n_skipped += (unsigned long long)(kn - k);
                k = kn;
                continue;
            }
        }
        const float s = tri(v, d, x, y, z);
        n_taken++;
        const int i0 = min((int)s, nt - 2);
        const float f = s - (float)i0;
        const float4 e0 = table[i0], e1 = table[i0 + 1];
        const float a = lerpf(e0.w, e1.w, f);
        if (a > 0.0f) {
            float cr = lerpf(e0.x, e1.x, f), cg = lerpf(e0.y, e1.y, f), cb = lerpf(e0.z, e1.z, f);
            if (p.shade) shade_at(v, d, l, x, y, z, cr, cg, cb);
            const float w = (1.0f - A) * a;
            ar += w * cr;
            ag += w * cg;
            ab += w * cb;
            A += w;
            if (A >= OPAQUE) {
                n_early = 1;
                break;
            }
        }
        k++;
    }
    r = ar + (1.0f - A) * r;
    g = ag + (1.0f - A) * g;
    b = ab + (1.0f - A) * b;
}

// pixel (px, py) of the viewport: float RGBA, or with p.out_u8 bytes floor(255 v + 0.5) clamped
__device__ __forceinline__ void write_pixel(void *out, const ivx_volren_params &p, int px, int py, float r, float g,
                                            float b, float A) {
    const int64_t o = ((int64_t)py * p.width + px) * 4;
    if (p.out_u8) {
        uint8_t *q = (uint8_t *)out + o;
        const float vals[4] = {r, g, b, A};
        for (int i = 0; i < 4; i++) q[i] = (uint8_t)clampf(floorf(255.0f * vals[i] + 0.5f), 0.0f, 255.0f);
    } else {
        float *q = (float *)out + o;
        q[0] = r;
        q[1] = g;
        q[2] = b;
        q[3] = A;
    }
}

// the wave's counts into stats[0..3]: samples taken, samples skipped, rays ended early, rays that meet the box
__device__ __forceinline__ void add_stats(unsigned long long *stats, unsigned long long taken, unsigned long long skipped,
                                          unsigned long long early, unsigned long long hit) {
    if (!stats) return;
    taken = wave_sum(taken);
    skipped = wave_sum(skipped);
    early = wave_sum(early);
    hit = wave_sum(hit);
    if (threadIdx.x == 0) {
        atomicAdd(stats + 0, taken);
        atomicAdd(stats + 1, skipped);
        atomicAdd(stats + 2, early);
        atomicAdd(stats + 3, hit);
    }
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
