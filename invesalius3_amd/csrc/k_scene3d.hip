// k_scene3d.hip -- the 3-D scene: the ray-cast field, the surfaces and the three slice planes in one picture (the reference's
// 3-D viewer: both volume mappers with IntermixIntersectingGeometryOn, invesalius/data/volume.py:644 and volume_mask.py:52, the
// surface actors, and viewer_volume.SlicePlane's textured planes).  One ray per pixel carries the field's front-to-back composite
// and blends every surface and plane fragment at its depth: a fragment at depth t goes before sample
// K_f = ceil((t - tin) / dt), between two fragments the loop is volren_ray.h's composite loop, so a field alone gives
// ivx_dev_volren_render / ivx_dev_maskren_render bit for bit and opaque surfaces alone ivx_dev_surface_resolve.
//
// MI355X design: latency-bound gathers like the two ray casters, no MFMA.  One wave per 8 x 8 pixel tile, a lane per ray.  The
// layer and plane table comes in the kernel arguments and is indexed per lane from LDS.  A lane reads its <= 8 keys
// (ivx_dev_surface_raster's, unchanged), computes its <= 3 plane hits, and then picks the nearest remaining fragment over
// eleven registers (scene3d_math.h, the resolve's selection), marches the field up to the fragment's sample with the segment form
// of composite_ray, shades the fragment with surfview_math.h and blends it.  A jump over an empty macro cell lands on
// min(cell exit, K_f), so skipping changes no bit.
#include <cmath>

#include "ivx_internal.h"
#include "volren_ray.h"
#include "surfview_math.h"
#include "scene3d_math.h"

using namespace ivx;

namespace {

using namespace ivx_scene3d;

struct SceneArgs {
    ivx_surface_camera cam;
    ivx_surface_layer layers[IVX_SURFACE_MAX_LAYERS];
    ivx_scene_plane planes[IVX_SCENE_MAX_PLANES]; // by orientation; picture null: no plane
    ivx_volren_params p;
    Dims d, c;
    int nlayers, mode, off;
    const float4 *table;
    const uint32_t *prefix;
    void *out;
    unsigned long long *stats;
};

// composite_ray's loop over the samples k .. kend - 1 with the sums carried: the same operations in the same order, a jump
// capped at kend.  True when the ray ended (A >= OPAQUE).
template <class F>
__device__ __forceinline__ bool march_segment(const F &v, const typename F::cell_t *__restrict__ cells, const Dims &d, const Dims &c,
                                              const float4 *__restrict__ table, const uint32_t *__restrict__ prefix,
                                              const ivx_volren_params &p, const Light &l, const RayCtx &ray, long long &k,
                                              long long kend, float &ar, float &ag, float &ab, float &A,
                                              unsigned long long &n_taken, unsigned long long &n_skipped) {
    const int nt = p.n_table;
    while (k < kend) {
        float x, y, z;
        sample_pos(ray, d, k, x, y, z);
        if (p.skip) {
            const int cx = (int)x / CELL, cy = (int)y / CELL, cz = (int)z / CELL;
            const int64_t ci = ((int64_t)cz * c.ny + cy) * c.nx + cx;
            if (F::transparent(prefix, nt, (int)cells[2 * ci], (int)cells[2 * ci + 1])) {
                long long kn = cell_exit(ray, d, k, cx, cy, cz);
                if (kn > kend) kn = kend;
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
            if (A >= OPAQUE) return true;
        }
        k++;
    }
    return false;
}

template <class F, bool HAS_FIELD>
__global__ __launch_bounds__(64) void k_scene_render(F v, const typename F::cell_t *__restrict__ cells, SceneArgs a) {
    __shared__ ivx_surface_layer s_layers[IVX_SURFACE_MAX_LAYERS];
    __shared__ ivx_scene_plane s_planes[IVX_SCENE_MAX_PLANES];
#pragma unroll
    for (int k = 0; k < IVX_SURFACE_MAX_LAYERS; k++)
        if (threadIdx.x == (unsigned)k) s_layers[k] = a.layers[k];
#pragma unroll
    for (int k = 0; k < IVX_SCENE_MAX_PLANES; k++)
        if (threadIdx.x == (unsigned)(IVX_SURFACE_MAX_LAYERS + k)) s_planes[k] = a.planes[k];
    __syncthreads();
    const ivx_volren_params &p = a.p;
    const int px = blockIdx.x * TILE + (threadIdx.x & (TILE - 1));
    const int py = blockIdx.y * TILE + (threadIdx.x / TILE);
    const bool active = px < p.width && py < p.height;
    unsigned long long n_taken = 0, n_skipped = 0, n_early = 0, n_hit = 0;
    if (active) {
        RayCtx ray;
        bool hit = false;
        if (HAS_FIELD) hit = setup_ray(p, a.d, px, py, ray);
        if (!hit) {
            ray.kmax = -1;
            ray.tin = 0.0;
        }
        n_hit = hit ? 1 : 0;
        // the fragments: (ord depth << 32) | layer, all ones where the layer has nothing here
        uint64_t sk[MAX_FRAGS];
        uint32_t tri_of[IVX_SURFACE_MAX_LAYERS];
        float pu[IVX_SCENE_MAX_PLANES], pv[IVX_SCENE_MAX_PLANES];
        const int64_t pix = (int64_t)py * p.width + px;
#pragma unroll
        for (int k = 0; k < IVX_SURFACE_MAX_LAYERS; k++) {
            sk[k] = KEY_EMPTY;
            tri_of[k] = 0;
            if (k < a.nlayers) {
                const uint64_t key = s_layers[k].keys[pix];
                if (key != KEY_EMPTY) {
                    sk[k] = (key & 0xffffffff00000000ull) | (uint64_t)k;
                    tri_of[k] = (uint32_t)key;
                }
            }
        }
        double P0[3];
        for (int q = 0; q < 3; q++) P0[q] = p.origin[q] + (double)px * p.du[q] + (double)py * p.dv[q];
#pragma unroll
        for (int o = 0; o < IVX_SCENE_MAX_PLANES; o++) {
            sk[IVX_SURFACE_MAX_LAYERS + o] = KEY_EMPTY;
            pu[o] = pv[o] = 0.0f;
            float t;
            if (s_planes[o].picture && plane_hit(P0, p.dir, p.spacing, o, s_planes[o].slice, s_planes[o].h, s_planes[o].w, a.off, t, pu[o], pv[o]))
                sk[IVX_SURFACE_MAX_LAYERS + o] = frag_key(t, IVX_SURFACE_MAX_LAYERS + o);
        }
        Light l;
        if (HAS_FIELD) l = make_light(p, a.d);
        float ar = 0.0f, ag = 0.0f, ab = 0.0f, A = 0.0f;
        long long k = 0;
        uint64_t prev = 0;
        bool first = true;
        for (;;) { // near to far: the field up to the fragment's sample, then the fragment; at last the rest of the field
            uint64_t m;
            const bool frag = next_fragment(sk, first, prev, m);
            if (HAS_FIELD && hit) {
                const long long kend = frag ? frag_sample(key_depth(m), ray.tin, p.dt, ray.kmax) : ray.kmax + 1;
                if (march_segment(v, cells, a.d, a.c, a.table, a.prefix, p, l, ray, k, kend, ar, ag, ab, A, n_taken, n_skipped)) {
                    n_early = 1;
                    break;
                }
            }
            if (!frag) break;
            prev = m;
            first = false;
            const int layer = (int)(m & LAYER_MASK);
            float c[3], alpha;
            if (layer < IVX_SURFACE_MAX_LAYERS) {
                uint32_t mt = 0;
#pragma unroll
                for (int q = 0; q < IVX_SURFACE_MAX_LAYERS; q++)
                    if (q == layer) mt = tri_of[q];
                const ivx_surface_layer &L = s_layers[layer];
                double I;
                if (!ivx_surfview::shade(a.cam, L, mt, px, py, a.mode, I)) continue;
                for (int q = 0; q < 3; q++) c[q] = (float)((double)L.rgb[q] * I);
                alpha = L.opacity;
            } else {
                const int o = layer - IVX_SURFACE_MAX_LAYERS;
                float u = 0.0f, w = 0.0f;
#pragma unroll
                for (int q = 0; q < IVX_SCENE_MAX_PLANES; q++)
                    if (q == o) u = pu[q], w = pv[q];
                const ivx_scene_plane &P = s_planes[o];
                plane_texel(P.picture, P.h, P.w, u, w, c);
                alpha = P.opacity;
            }
            const float w = (1.0f - A) * alpha;
            ar += w * c[0];
            ag += w * c[1];
            ab += w * c[2];
            A += w;
            if (A >= OPAQUE) {
                n_early = 1;
                break;
            }
        }
        const float r = ar + (1.0f - A) * (float)p.background[0];
        const float g = ag + (1.0f - A) * (float)p.background[1];
        const float b = ab + (1.0f - A) * (float)p.background[2];
        write_pixel(a.out, p, px, py, r, g, b, A);
    }
    add_stats(a.stats, n_taken, n_skipped, n_early, n_hit);
}

static inline size_t al256(size_t x) { return (x + 255) & ~(size_t)255; }

int check_scene_args(int field_kind, const ivx_surface_layer *layers, int nlayers, const ivx_surface_camera *cam, int interpolation,
                     const ivx_scene_plane *planes, int nplanes, const ivx_volren_params *p, const void *out) {
    int rc;
    if ((rc = check_params(p))) return rc;
    IVX_REQUIRE(field_kind >= IVX_SCENE_FIELD_NONE && field_kind <= IVX_SCENE_FIELD_MASK, IVX_EINVAL, "scene: field kind %d", field_kind);
    IVX_REQUIRE(!p->mip, IVX_EINVAL, "scene: no maximum intensity mode (composite fields only)");
    IVX_REQUIRE(field_kind != IVX_SCENE_FIELD_MASK || !p->clip, IVX_EINVAL, "scene: no clip plane on the mask field");
    IVX_REQUIRE(cam && out, IVX_EINVAL, "scene: null camera / picture");
    IVX_REQUIRE(cam->width == p->width && cam->height == p->height, IVX_EINVAL, "scene: camera viewport %d x %d, params %d x %d",
                cam->width, cam->height, p->width, p->height);
    IVX_REQUIRE(cam->parallel_scale > 0.0 && cam->parallel_scale < INFINITY, IVX_EINVAL, "scene: parallel scale %g", cam->parallel_scale);
    for (int q = 0; q < 3; q++)
        IVX_REQUIRE(std::isfinite(cam->focal[q]) && std::isfinite(cam->right[q]) && std::isfinite(cam->up[q]) && std::isfinite(cam->dir[q]),
                    IVX_EINVAL, "scene: a camera number that is not finite");
    IVX_REQUIRE(nlayers >= 0 && nlayers <= IVX_SURFACE_MAX_LAYERS, IVX_EINVAL, "scene: %d surfaces (at most %d)", nlayers,
                IVX_SURFACE_MAX_LAYERS);
    IVX_REQUIRE(nplanes >= 0 && nplanes <= IVX_SCENE_MAX_PLANES, IVX_EINVAL, "scene: %d slice planes (at most %d)", nplanes,
                IVX_SCENE_MAX_PLANES);
    IVX_REQUIRE((nlayers == 0 || layers) && (nplanes == 0 || planes), IVX_EINVAL, "scene: null layers / planes");
    IVX_REQUIRE(interpolation >= IVX_SURFACE_FLAT && interpolation <= IVX_SURFACE_PHONG, IVX_EINVAL, "scene: interpolation %d", interpolation);
    for (int k = 0; k < nlayers; k++) {
        const ivx_surface_layer &L = layers[k];
        IVX_REQUIRE(L.nverts >= 0 && L.ntris >= 0 && L.nverts < 0x7fffffffll && L.ntris < 0x7fffffffll, IVX_EINVAL,
                    "scene: size of surface %d", k);
        IVX_REQUIRE(L.ntris == 0 || (L.verts && L.faces), IVX_EINVAL, "scene: surface %d has no arrays", k);
        IVX_REQUIRE(L.opacity >= 0.0f && L.opacity <= 1.0f, IVX_EINVAL, "scene: opacity %g of surface %d", (double)L.opacity, k);
        for (int q = 0; q < 3; q++)
            IVX_REQUIRE(L.rgb[q] >= 0.0f && L.rgb[q] <= 1.0f, IVX_EINVAL, "scene: colour %g of surface %d", (double)L.rgb[q], k);
    }
    int seen = 0;
    for (int k = 0; k < nplanes; k++) {
        const ivx_scene_plane &P = planes[k];
        IVX_REQUIRE(P.orientation >= IVX_SCENE_AXIAL && P.orientation <= IVX_SCENE_SAGITAL, IVX_EINVAL, "scene: orientation %d of plane %d",
                    P.orientation, k);
        IVX_REQUIRE(!(seen & (1 << P.orientation)), IVX_EINVAL, "scene: two planes of orientation %d", P.orientation);
        seen |= 1 << P.orientation;
        IVX_REQUIRE(P.picture && P.h >= 1 && P.w >= 1 && P.h <= 32768 && P.w <= 32768, IVX_EINVAL, "scene: picture of plane %d (%d x %d)", k,
                    P.h, P.w);
        IVX_REQUIRE(P.slice >= -32768 && P.slice <= 32768, IVX_EINVAL, "scene: slice %d of plane %d", P.slice, k);
        IVX_REQUIRE(P.opacity >= 0.0f && P.opacity <= 1.0f, IVX_EINVAL, "scene: opacity %g of plane %d", (double)P.opacity, k);
    }
    return IVX_OK;
}

} // namespace

extern "C" int ivx_dev_scene_render(int field_kind, const void *field, const void *cells, const int64_t shape[3],
                                    const int64_t strides[3], int apron, int apron_value, const float *table, const uint32_t *prefix,
                                    const ivx_surface_layer *layers, int nlayers, const ivx_surface_camera *cam, int interpolation,
                                    const ivx_scene_plane *planes, int nplanes, const ivx_volren_params *p, void *out, uint64_t *stats,
                                    void *stream) {
    int rc;
    if ((rc = check_scene_args(field_kind, layers, nlayers, cam, interpolation, planes, nplanes, p, out))) return rc;
    SceneArgs A;
    memset(&A, 0, sizeof(A));
    A.cam = *cam;
    for (int k = 0; k < nlayers; k++) {
        IVX_REQUIRE(layers[k].keys != nullptr, IVX_EINVAL, "scene: surface %d has no keys", k);
        A.layers[k] = layers[k];
    }
    for (int k = 0; k < nplanes; k++) A.planes[planes[k].orientation] = planes[k];
    A.p = *p;
    A.nlayers = nlayers;
    A.mode = interpolation;
    A.off = field_kind == IVX_SCENE_FIELD_MASK ? 1 : 0;
    A.table = (const float4 *)table;
    A.prefix = prefix;
    A.out = out;
    A.stats = (unsigned long long *)stats;
    const dim3 grid((unsigned)cdiv(p->width, TILE), (unsigned)cdiv(p->height, TILE)), block(TILE * TILE);
    hipStream_t st = S(stream);
    if (field_kind == IVX_SCENE_FIELD_NONE) {
        const DenseField f{nullptr, 0, 0};
        hipLaunchKernelGGL((k_scene_render<DenseField, false>), grid, block, 0, st, f, (const uint16_t *)nullptr, A);
        IVX_LAUNCH_CHECK();
        return IVX_OK;
    }
    IVX_REQUIRE(field && table, IVX_EINVAL, "scene: null field / table");
    IVX_REQUIRE(!p->skip || (cells && prefix), IVX_EINVAL, "scene: skipping needs the cells and the prefix counts");
    if (field_kind == IVX_SCENE_FIELD_IMAGE) {
        if ((rc = check_shape(shape, A.d))) return rc;
        A.c = cell_dims(A.d);
        const DenseField f{(const uint16_t *)field, (int64_t)A.d.ny * A.d.nx, A.d.nx};
        hipLaunchKernelGGL((k_scene_render<DenseField, true>), grid, block, 0, st, f, (const uint16_t *)cells, A);
    } else {
        IVX_REQUIRE(shape && strides, IVX_EINVAL, "scene: null shape / strides");
        IVX_REQUIRE(apron == 0 || apron == 1, IVX_EINVAL, "scene: apron %d (0 or 1)", apron);
        IVX_REQUIRE(apron_value >= 0 && apron_value <= 255, IVX_EINVAL, "scene: apron value %d", apron_value);
        IVX_REQUIRE(p->n_table >= 257, IVX_EINVAL, "scene: n_table %d (a byte reads entries 0 .. 256)", p->n_table);
        for (int q = 0; q < 3; q++) IVX_REQUIRE(shape[q] >= 1, IVX_EINVAL, "scene: shape[%d] = %lld", q, (long long)shape[q]);
        const int64_t logical[3] = {shape[0] + apron, shape[1] + apron, shape[2] + apron};
        if ((rc = check_shape(logical, A.d))) return rc;
        A.c = cell_dims(A.d);
        Field f;
        f.base = (const uint8_t *)field;
        f.sz = strides[0], f.sy = strides[1], f.sx = strides[2];
        f.apron = apron;
        f.av = (unsigned)apron_value;
        hipLaunchKernelGGL((k_scene_render<Field, true>), grid, block, 0, st, f, (const uint8_t *)cells, A);
    }
    IVX_LAUNCH_CHECK();
    return IVX_OK;
}

extern "C" int ivx_scene_render(int field_kind, const void *field, const int64_t shape[3], const int64_t strides[3], int shift,
                                int nsmooth, const float *table, const uint32_t *prefix, const ivx_surface_layer *layers, int nlayers,
                                const ivx_surface_camera *cam, int interpolation, const ivx_scene_plane *planes, int nplanes,
                                const ivx_volren_params *p, void *out) {
    HostCallGuard guard;
    int rc;
    if ((rc = check_scene_args(field_kind, layers, nlayers, cam, interpolation, planes, nplanes, p, out))) return rc;
    const size_t npix = (size_t)p->width * p->height;
    const size_t ob = npix * 4 * (p->out_u8 ? 1 : 4);
    void *d_out, *d_vol = nullptr, *d_cells = nullptr, *d_lut = nullptr;
    if ((rc = ws_get(WS_OUT, ob, &d_out))) return rc;
    const size_t nt = (size_t)p->n_table, tb = nt * 16, pb = (nt + 1) * 4;
    const int64_t *dense_strides = nullptr;
    int64_t dense[3] = {0, 0, 0};
    if (field_kind != IVX_SCENE_FIELD_NONE) {
        Dims d;
        if ((rc = check_shape(shape, d))) return rc;
        IVX_REQUIRE(field && strides && table && prefix, IVX_EINVAL, "scene: null buffer");
        const int64_t n = (int64_t)d.nz * d.ny * d.nx;
        const Dims c = cell_dims(d);
        const size_t ncell = (size_t)c.nz * c.ny * c.nx;
        if ((rc = ws_get(WS_LUT, tb + pb, &d_lut))) return rc;
        if ((rc = copy_h2d(d_lut, table, tb)) || (rc = copy_h2d((char *)d_lut + tb, prefix, pb))) return rc;
        if (field_kind == IVX_SCENE_FIELD_IMAGE) {
            void *d_in, *d_s;
            if ((rc = ws_get(WS_IN, (size_t)n * 2, &d_in)) || (rc = ws_get(WS_AUX0, (size_t)n * 2, &d_vol)) ||
                (rc = ws_get(WS_AUX1, (size_t)n * 2, &d_s)) || (rc = ws_get(WS_AUX2, ncell * 4, &d_cells)))
                return rc;
            if ((rc = upload_strided(d_in, field, shape, strides, 2, WS_IN))) return rc;
            if ((rc = ivx_dev_volren_prepare((const int16_t *)d_in, shape, shift, nsmooth, (uint16_t *)d_vol, (uint16_t *)d_s, nullptr)))
                return rc;
            if ((rc = ivx_dev_volren_cells((const uint16_t *)d_vol, shape, (uint16_t *)d_cells, nullptr))) return rc;
        } else {
            if ((rc = ws_get(WS_IN, (size_t)n, &d_vol)) || (rc = ws_get(WS_AUX2, ncell * 2, &d_cells))) return rc;
            if ((rc = upload_strided(d_vol, field, shape, strides, 1, WS_IN))) return rc;
            dense[0] = (int64_t)d.ny * d.nx, dense[1] = d.nx, dense[2] = 1;
            dense_strides = dense;
            if ((rc = ivx_dev_maskren_cells((const uint8_t *)d_vol, shape, dense, 0, 0, 0, -1, (uint8_t *)d_cells, nullptr))) return rc;
        }
    }
    // WS_AUX3: per surface [points][triangles][normals][keys], then the planes' pictures
    size_t total = 0;
    for (int k = 0; k < nlayers; k++) {
        const ivx_surface_layer &L = layers[k];
        for (int64_t q = 0; q < 3 * L.ntris; q++)
            IVX_REQUIRE(L.faces[q] >= 0 && L.faces[q] < L.nverts, IVX_EDOM, "scene: surface %d: face index %d outside [0, %lld)", k,
                        L.faces[q], (long long)L.nverts);
        total += al256((size_t)L.nverts * 12 + 16) * (L.normals ? 2 : 1) + al256((size_t)L.ntris * 12 + 16) + al256(npix * 8);
    }
    for (int k = 0; k < nplanes; k++) total += al256((size_t)planes[k].h * planes[k].w * 3);
    void *d_geo;
    if ((rc = ws_get(WS_AUX3, total + 256, &d_geo))) return rc;
    ivx_surface_layer dl[IVX_SURFACE_MAX_LAYERS];
    ivx_scene_plane dp[IVX_SCENE_MAX_PLANES];
    char *w = (char *)d_geo;
    for (int k = 0; k < nlayers; k++) {
        const ivx_surface_layer &L = layers[k];
        dl[k] = L;
        dl[k].verts = (const float *)w;
        if ((rc = copy_h2d(w, L.verts, (size_t)L.nverts * 12))) return rc;
        w += al256((size_t)L.nverts * 12 + 16);
        dl[k].faces = (const int32_t *)w;
        if ((rc = copy_h2d(w, L.faces, (size_t)L.ntris * 12))) return rc;
        w += al256((size_t)L.ntris * 12 + 16);
        if (L.normals) {
            dl[k].normals = (const float *)w;
            if ((rc = copy_h2d(w, L.normals, (size_t)L.nverts * 12))) return rc;
            w += al256((size_t)L.nverts * 12 + 16);
        }
        dl[k].keys = (const uint64_t *)w;
        if ((rc = ivx_dev_surface_raster(dl[k].verts, L.nverts, dl[k].faces, L.ntris, cam, IVX_RASTER_ALL, (uint64_t *)w, nullptr))) return rc;
        w += al256(npix * 8);
    }
    for (int k = 0; k < nplanes; k++) {
        dp[k] = planes[k];
        dp[k].picture = (const uint8_t *)w;
        if ((rc = copy_h2d(w, planes[k].picture, (size_t)planes[k].h * planes[k].w * 3))) return rc;
        w += al256((size_t)planes[k].h * planes[k].w * 3);
    }
    if ((rc = ivx_dev_scene_render(field_kind, d_vol, d_cells, shape, dense_strides, 0, 0, (const float *)d_lut,
                                   d_lut ? (const uint32_t *)((char *)d_lut + tb) : nullptr, dl, nlayers, cam, interpolation, dp, nplanes, p,
                                   d_out, nullptr, nullptr)))
        return rc;
    IVX_HIP(hipDeviceSynchronize());
    return copy_d2h(out, d_out, ob);
}
