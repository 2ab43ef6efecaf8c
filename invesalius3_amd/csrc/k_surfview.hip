// k_surfview.hip -- the surface view (Surface._show_surface, invesalius/data/surface.py:1061-1116: a vtkPolyDataMapper and a
// vtkActor with back-face culling, a colour, an opacity and an interpolation mode under the parallel camera of the 3-D viewer)
// as a software rasteriser: meshes in, a shaded RGBA picture out.  The rules make the picture a function of the input
// alone: float64 + - * / sqrt in one stated order (-ffp-contract=off), edge functions from the smaller vertex id (meshvis_math.h),
// depth rounded to float32 once, and the nearest fragment kept by ONE unsigned 64-bit atomic minimum on (ordered depth, triangle
// index) -- equal depths go to the lower index, so the key buffer does not depend on the order the triangles arrive in.
//
// MI355X design: byte-bound streams plus an 8-byte scatter, no MFMA.
//   clear    8 bytes per pixel of all ones, plain stores; the queue's counter <- 0
//   raster   the two-kernel shape of k_meshvis.hip: lane per triangle walks a box of up to IVX_RASTER_SMALL_BOX pixels, a larger
//            box is queued (one atomic add) for a workgroup of 256 lanes that strides it.  A plain load screens the atomic.
//   resolve  lane per pixel: the <= 8 keys, then per surviving fragment 84 bytes of gathers (three ids, three points, three
//            normals), the shading, the blend far to near; 16 or 4 bytes out plus the optional ids and depth.  The layer table
//            comes in the kernel arguments and is indexed per lane from LDS.
#include <algorithm>
#include <cmath>

#include "ivx_internal.h"
#include "surfview_math.h"

namespace {

using namespace ivx_surfview;

__global__ __launch_bounds__(256) void k_sv_clear(uint64_t *__restrict__ keys, int64_t npix, uint32_t *__restrict__ nqueued) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < npix; p += stride) keys[p] = KEY_EMPTY;
    if (blockIdx.x == 0 && threadIdx.x == 0) *nqueued = 0u;
}

__device__ __forceinline__ void key_pixel(const Tri &T, int i, int j, int width, uint32_t tri, uint64_t *__restrict__ keys) {
    uint64_t key;
    if (!pixel_key(T, i, j, tri, key)) return;
    unsigned long long *cell = (unsigned long long *)(keys + (int64_t)j * width + i);
    if (key < *cell) atomicMin(cell, (unsigned long long)key);
}

__global__ __launch_bounds__(256) void k_sv_raster_small(const float *__restrict__ verts, int64_t nverts,
                                                         const int32_t *__restrict__ faces, int64_t ntris, ivx_surface_camera C,
                                                         uint64_t *__restrict__ keys, uint32_t *__restrict__ queue,
                                                         uint32_t *__restrict__ nqueued) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= ntris) return;
    Tri T;
    if (!load_tri(C, verts, nverts, faces, t, T)) return;
    const int64_t box = (int64_t)(T.x1 - T.x0 + 1) * (T.y1 - T.y0 + 1);
    if (box > IVX_RASTER_SMALL_BOX) {
        const uint32_t q = atomicAdd(nqueued, 1u); // at most ntris entries after a clear
        if ((int64_t)q < ntris) queue[q] = (uint32_t)t; // (a counter nobody cleared must not lead anywhere)
        return;
    }
    for (int j = T.y0; j <= T.y1; j++)
        for (int i = T.x0; i <= T.x1; i++) key_pixel(T, i, j, C.width, (uint32_t)t, keys);
}

__global__ __launch_bounds__(256) void k_sv_raster_big(const float *__restrict__ verts, int64_t nverts,
                                                       const int32_t *__restrict__ faces, int64_t ntris, ivx_surface_camera C,
                                                       uint64_t *__restrict__ keys, const uint32_t *__restrict__ queue,
                                                       const uint32_t *__restrict__ nqueued) {
    const uint32_t n = (uint32_t)min((int64_t)*nqueued, ntris); // (a queue nobody cleared must not lead anywhere)
    for (uint32_t q = blockIdx.x; q < n; q += gridDim.x) {
        const int64_t t = (int64_t)queue[q];
        Tri T;
        if (t >= ntris || !load_tri(C, verts, nverts, faces, t, T)) continue; // (it passed once already)
        const uint32_t bw = (uint32_t)(T.x1 - T.x0 + 1);
        const uint32_t box = bw * (uint32_t)(T.y1 - T.y0 + 1); // < 2^31: check_camera
        for (uint32_t k = threadIdx.x; k < box; k += 256) key_pixel(T, T.x0 + (int)(k % bw), T.y0 + (int)(k / bw), C.width, (uint32_t)t, keys);
    }
}

struct ResolveArgs {
    ivx_surface_camera cam;
    ivx_surface_layer layers[IVX_SURFACE_MAX_LAYERS];
    float background[3];
    int nlayers, mode, out_u8;
    void *rgba;
    int32_t *ids;
    float *depth;
};

__global__ __launch_bounds__(256) void k_sv_resolve(ResolveArgs A) {
    __shared__ ivx_surface_layer s_layers[IVX_SURFACE_MAX_LAYERS];
#pragma unroll
    for (int k = 0; k < IVX_SURFACE_MAX_LAYERS; k++)
        if (threadIdx.x == (unsigned)k) s_layers[k] = A.layers[k];
    __syncthreads();
    const int64_t pix = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (pix >= (int64_t)A.cam.width * A.cam.height) return;
    float rgba[4], t;
    int32_t id[2];
    resolve_pixel(A.cam, s_layers, A.nlayers, A.mode, A.background, (int)(pix % A.cam.width), (int)(pix / A.cam.width), rgba, id, &t);
    if (A.out_u8)
        ((uchar4 *)A.rgba)[pix] = make_uchar4(to_u8(rgba[0]), to_u8(rgba[1]), to_u8(rgba[2]), to_u8(rgba[3]));
    else
        ((float4 *)A.rgba)[pix] = make_float4(rgba[0], rgba[1], rgba[2], rgba[3]);
    if (A.ids) ((int2 *)A.ids)[pix] = make_int2(id[0], id[1]);
    if (A.depth) A.depth[pix] = t;
}

static inline size_t al256(size_t x) { return (x + 255) & ~(size_t)255; }

static int check_camera(const ivx_surface_camera *c) {
    IVX_REQUIRE(c != nullptr, IVX_EINVAL, "surface camera: null");
    IVX_REQUIRE(c->width > 0 && c->height > 0 && (int64_t)c->width * c->height < 0x7fffffffll, IVX_EINVAL,
                "surface camera: viewport %d x %d", c->width, c->height);
    IVX_REQUIRE(c->parallel_scale > 0.0 && c->parallel_scale < INFINITY, IVX_EINVAL, "surface camera: parallel scale %g",
                c->parallel_scale);
    for (int q = 0; q < 3; q++)
        IVX_REQUIRE(std::isfinite(c->focal[q]) && std::isfinite(c->right[q]) && std::isfinite(c->up[q]) && std::isfinite(c->dir[q]),
                    IVX_EINVAL, "surface camera: a number that is not finite");
    return IVX_OK;
}
static int check_mesh_sizes(int64_t nverts, int64_t ntris) {
    IVX_REQUIRE(nverts >= 0 && ntris >= 0, IVX_EINVAL, "surface: negative size");
    IVX_REQUIRE(nverts < 0x7fffffffll && ntris < 0x7fffffffll, IVX_EINVAL, "surface: more than 2^31 vertices / triangles");
    return IVX_OK;
}
static int check_scene(const ivx_surface_layer *layers, int nlayers, const ivx_surface_camera *cam, int interpolation,
                       const float *background, const void *rgba) {
    int rc;
    if ((rc = check_camera(cam))) return rc;
    IVX_REQUIRE(nlayers >= 0 && nlayers <= IVX_SURFACE_MAX_LAYERS, IVX_EINVAL, "surface view: %d surfaces (at most %d)", nlayers,
                IVX_SURFACE_MAX_LAYERS);
    IVX_REQUIRE(nlayers == 0 || layers != nullptr, IVX_EINVAL, "surface view: null layers");
    IVX_REQUIRE(interpolation >= IVX_SURFACE_FLAT && interpolation <= IVX_SURFACE_PHONG, IVX_EINVAL, "surface view: interpolation %d",
                interpolation);
    IVX_REQUIRE(background && rgba, IVX_EINVAL, "surface view: null background / picture");
    for (int q = 0; q < 3; q++) IVX_REQUIRE(std::isfinite(background[q]), IVX_EINVAL, "surface view: background is not finite");
    for (int k = 0; k < nlayers; k++) {
        const ivx_surface_layer &L = layers[k];
        if ((rc = check_mesh_sizes(L.nverts, L.ntris))) return rc;
        IVX_REQUIRE(L.ntris == 0 || (L.verts && L.faces), IVX_EINVAL, "surface view: surface %d has no arrays", k);
        IVX_REQUIRE(L.opacity >= 0.0f && L.opacity <= 1.0f, IVX_EINVAL, "surface view: opacity %g of surface %d", (double)L.opacity, k);
        for (int q = 0; q < 3; q++)
            IVX_REQUIRE(L.rgb[q] >= 0.0f && L.rgb[q] <= 1.0f, IVX_EINVAL, "surface view: colour %g of surface %d", (double)L.rgb[q], k);
    }
    return IVX_OK;
}

} // namespace

extern "C" int ivx_dev_surface_raster(const float *verts, int64_t nverts, const int32_t *faces, int64_t ntris,
                                      const ivx_surface_camera *cam, int stages, uint64_t *keys, void *stream) {
    int rc;
    if ((rc = check_mesh_sizes(nverts, ntris)) || (rc = check_camera(cam))) return rc;
    IVX_REQUIRE(stages > 0 && stages <= IVX_RASTER_ALL, IVX_EINVAL, "surface raster: stages %d", stages);
    IVX_REQUIRE(keys != nullptr && (ntris == 0 || (verts && faces)), IVX_EINVAL, "surface raster: null array");
    hipStream_t st = ivx::S(stream);
    // per-stream WS_MESH2: [queue: ntris words][counter]
    const size_t off_count = al256((size_t)ntris * 4 + 4);
    void *ws;
    if ((rc = ivx::ws_get_s(ivx::WS_MESH2, st, off_count + 256, &ws))) return rc;
    uint32_t *queue = (uint32_t *)ws, *count = (uint32_t *)((char *)ws + off_count);
    const int64_t npix = (int64_t)cam->width * cam->height;
    if (stages & IVX_RASTER_CLEAR) {
        hipLaunchKernelGGL(k_sv_clear, dim3((unsigned)std::min<int64_t>(ivx::cdiv(npix, 256), 4096)), dim3(256), 0, st, keys, npix, count);
        IVX_LAUNCH_CHECK();
    }
    if (ntris == 0) return IVX_OK; // (no launch with an empty grid)
    if (stages & IVX_RASTER_SMALL) {
        hipLaunchKernelGGL(k_sv_raster_small, dim3((unsigned)ivx::cdiv(ntris, 256)), dim3(256), 0, st, verts, nverts, faces, ntris, *cam,
                           keys, queue, count);
        IVX_LAUNCH_CHECK();
    }
    if (stages & IVX_RASTER_BIG) {
        hipLaunchKernelGGL(k_sv_raster_big, dim3((unsigned)std::min<int64_t>(ntris, 2048)), dim3(256), 0, st, verts, nverts, faces, ntris,
                           *cam, keys, (const uint32_t *)queue, (const uint32_t *)count);
        IVX_LAUNCH_CHECK();
    }
    return IVX_OK;
}

extern "C" int ivx_dev_surface_resolve(const ivx_surface_layer *layers, int nlayers, const ivx_surface_camera *cam, int interpolation,
                                       const float *background, int out_u8, void *rgba, int32_t *ids, float *depth, void *stream) {
    int rc;
    if ((rc = check_scene(layers, nlayers, cam, interpolation, background, rgba))) return rc;
    ResolveArgs A;
    memset(&A, 0, sizeof(A));
    A.cam = *cam;
    for (int k = 0; k < nlayers; k++) {
        IVX_REQUIRE(layers[k].keys != nullptr, IVX_EINVAL, "surface view: surface %d has no keys", k);
        A.layers[k] = layers[k];
    }
    for (int q = 0; q < 3; q++) A.background[q] = background[q];
    A.nlayers = nlayers;
    A.mode = interpolation;
    A.out_u8 = out_u8 ? 1 : 0;
    A.rgba = rgba;
    A.ids = ids;
    A.depth = depth;
    const int64_t npix = (int64_t)cam->width * cam->height;
    hipLaunchKernelGGL(k_sv_resolve, dim3((unsigned)ivx::cdiv(npix, 256)), dim3(256), 0, ivx::S(stream), A);
    IVX_LAUNCH_CHECK();
    return IVX_OK;
}

extern "C" int ivx_surface_render(const ivx_surface_layer *layers, int nlayers, const ivx_surface_camera *cam, int interpolation,
                                  const float *background, int out_u8, void *rgba, int32_t *ids, float *depth) {
    ivx::HostCallGuard host_guard__;
    using namespace ivx;
    int rc;
    if ((rc = check_scene(layers, nlayers, cam, interpolation, background, rgba))) return rc;
    const size_t npix = (size_t)cam->width * cam->height;
    // WS_IN: per surface [points][triangles][normals][keys]; WS_OUT: [picture][ids][depth]
    size_t total = 0;
    for (int k = 0; k < nlayers; k++) {
        const ivx_surface_layer &L = layers[k];
        for (int64_t q = 0; q < 3 * L.ntris; q++)
            IVX_REQUIRE(L.faces[q] >= 0 && L.faces[q] < L.nverts, IVX_EDOM, "surface %d: face index %d outside [0, %lld)", k, L.faces[q],
                        (long long)L.nverts);
        total += al256((size_t)L.nverts * 12 + 16) * (L.normals ? 2 : 1) + al256((size_t)L.ntris * 12 + 16) + al256(npix * 8);
    }
    void *d_in, *d_out;
    if ((rc = ws_get(WS_IN, total + 256, &d_in))) return rc;
    const size_t pic = al256(npix * (out_u8 ? 4 : 16)), off_ids = pic, off_depth = pic + al256(npix * 8);
    if ((rc = ws_get(WS_OUT, off_depth + al256(npix * 4), &d_out))) return rc;
    ivx_surface_layer dl[IVX_SURFACE_MAX_LAYERS];
    char *w = (char *)d_in;
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
    char *o = (char *)d_out;
    if ((rc = ivx_dev_surface_resolve(dl, nlayers, cam, interpolation, background, out_u8, o, ids ? (int32_t *)(o + off_ids) : nullptr,
                                      depth ? (float *)(o + off_depth) : nullptr, nullptr)))
        return rc;
    IVX_HIP(hipDeviceSynchronize());
    if ((rc = copy_d2h(rgba, o, npix * (out_u8 ? 4 : 16)))) return rc;
    if (ids && (rc = copy_d2h(ids, o + off_ids, npix * 8))) return rc;
    if (depth && (rc = copy_d2h(depth, o + off_depth, npix * 4))) return rc;
    return IVX_OK;
}
