// k_meshvis.hip -- "Remove non-visible faces" (pu.RemoveNonVisibleFaces / pu.HasNonVisibleFaces,
// invesalius/data/polydata_utils.py:281-455) on the indexed mesh.  The reference renders the whole mesh off screen with OpenGL
// from six sides and asks vtkSelectVisiblePoints which points the z-buffer lets through; here that is a depth-only software
// rasteriser: mesh in, float32 z-buffer out, a point test against it, and the compaction k_mesh.hip already has.
// The rules are written so that the result is a function of the input alone: float64 + - * / in one stated order
// (-ffp-contract=off), every edge function evaluated from the smaller vertex id so that the two triangles on an edge see the
// same number, depth rounded to float32 once, minimum by an unsigned atomic on the float's bits (exact for depths >= 0).
//
// MI355X design: byte-bound streams plus a 4-byte scatter, no MFMA, no LDS staging.
//   bounds   grid-stride min/max, wave shuffle -> LDS -> per-workgroup partials -> one workgroup (exact, order-free)
//   raster   lane per triangle: project the three corners, clamp the pixel box; a box of up to IVX_RASTER_SMALL_BOX pixels is
//            walked by the lane (a real surface at 800 x 800 is almost all sub-pixel triangles: zero or one centre each), a larger
//            one is appended to a queue that a second kernel drains, one workgroup per triangle striding the box -- a 12-triangle
//            cube covers ~10^5 pixels per triangle.  A plain load screens the atomic: most candidates lose against what is there.
//   points   lane per point and view; a point some earlier view saw is skipped; one byte per point, plain stores
//   select   mark (any corner flagged) -> two exclusive scans -> the compaction of mesh_compact.h
#include <algorithm>

#include "ivx_internal.h"
#include "mesh_compact.h"
#include "meshvis_math.h"
#include "scan_u32.h"

namespace {

using namespace ivx_meshvis;

__device__ __forceinline__ void shade_pixel(const Tri &T, int i, int j, int width, uint32_t *__restrict__ depth) {
    uint32_t bits;
    if (!pixel_depth_bits(T, i, j, bits)) return;
    uint32_t *cell = depth + (int64_t)j * width + i;
    if (bits < *cell) atomicMin(cell, bits);
}

__global__ __launch_bounds__(256) void k_vis_raster_small(const float *__restrict__ verts, int64_t nverts,
                                                          const int32_t *__restrict__ faces, int64_t ntris, ivx_mesh_view V,
                                                          uint32_t *__restrict__ depth, uint32_t *__restrict__ queue,
                                                          uint32_t *__restrict__ nqueued) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= ntris) return;
    Tri T;
    if (!load_tri(V, verts, nverts, faces, t, T)) return;
    const int64_t box = (int64_t)(T.x1 - T.x0 + 1) * (T.y1 - T.y0 + 1);
    if (box > IVX_RASTER_SMALL_BOX) {
        queue[atomicAdd(nqueued, 1u)] = (uint32_t)t; // at most ntris entries
        return;
    }
    for (int j = T.y0; j <= T.y1; j++)
        for (int i = T.x0; i <= T.x1; i++) shade_pixel(T, i, j, V.width, depth);
}

__global__ __launch_bounds__(256) void k_vis_raster_big(const float *__restrict__ verts, int64_t nverts,
                                                        const int32_t *__restrict__ faces, int64_t ntris, ivx_mesh_view V,
                                                        uint32_t *__restrict__ depth, const uint32_t *__restrict__ queue,
                                                        const uint32_t *__restrict__ nqueued) {
    const uint32_t n = (uint32_t)min((int64_t)*nqueued, ntris); // (a queue nobody cleared must not lead anywhere)
    for (uint32_t q = blockIdx.x; q < n; q += gridDim.x) {
        const int64_t t = (int64_t)queue[q];
        Tri T;
        if (t >= ntris || !load_tri(V, verts, nverts, faces, t, T)) continue; // (it passed once already)
        const uint32_t bw = (uint32_t)(T.x1 - T.x0 + 1);
        const uint32_t box = bw * (uint32_t)(T.y1 - T.y0 + 1); // < 2^31: check_view
        for (uint32_t k = threadIdx.x; k < box; k += 256) shade_pixel(T, T.x0 + (int)(k % bw), T.y0 + (int)(k / bw), V.width, depth);
    }
}

__global__ __launch_bounds__(256) void k_vis_points(const float *__restrict__ verts, int64_t nverts, ivx_mesh_view V,
                                                    const float *__restrict__ depth, uint8_t *__restrict__ flags) {
    const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= nverts || flags[v]) return; // an earlier view saw it
    if (point_visible(V, verts + 3 * v, depth)) flags[v] = 1;
}

// ---- bounds ---------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void block_minmax(float lo[3], float hi[3], float *__restrict__ out6) {
    __shared__ float s_part[4][6];
#pragma unroll
    for (int q = 0; q < 3; q++) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            lo[q] = fminf(lo[q], __shfl_xor(lo[q], o, 64));
            hi[q] = fmaxf(hi[q], __shfl_xor(hi[q], o, 64));
        }
    }
    const int wv = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0)
        for (int q = 0; q < 3; q++) {
            s_part[wv][2 * q] = lo[q];
            s_part[wv][2 * q + 1] = hi[q];
        }
    __syncthreads();
    if (threadIdx.x < 6) {
        const int q = threadIdx.x;
        const float a = s_part[0][q], b = s_part[1][q], c = s_part[2][q], d = s_part[3][q];
        out6[q] = (q & 1) ? fmaxf(fmaxf(a, b), fmaxf(c, d)) : fminf(fminf(a, b), fminf(c, d));
    }
}
__global__ __launch_bounds__(256) void k_vis_bounds(const float *__restrict__ verts, int64_t nverts, float *__restrict__ partial) {
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; v < nverts; v += stride) {
#pragma unroll
        for (int q = 0; q < 3; q++) {
            const float c = verts[3 * v + q];
            lo[q] = fminf(lo[q], c);
            hi[q] = fmaxf(hi[q], c);
        }
    }
    block_minmax(lo, hi, partial + 6 * (int64_t)blockIdx.x);
}
__global__ __launch_bounds__(256) void k_vis_bounds_final(const float *__restrict__ partial, int nb, float *__restrict__ out6) {
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int b = threadIdx.x; b < nb; b += 256) {
#pragma unroll
        for (int q = 0; q < 3; q++) {
            lo[q] = fminf(lo[q], partial[6 * b + 2 * q]);
            hi[q] = fmaxf(hi[q], partial[6 * b + 2 * q + 1]);
        }
    }
    block_minmax(lo, hi, out6);
}

// ---- selection ------------------------------------------------------------------------------------------------------
// keep[t] = 1 when any corner of t is flagged (invert: when any corner is NOT flagged); used[v] = 1 for the kept corners
__global__ __launch_bounds__(256) void k_vis_mark(const int32_t *__restrict__ faces, int64_t ntris, int64_t nverts,
                                                  const uint8_t *__restrict__ flags, int invert, uint32_t *__restrict__ keep,
                                                  uint32_t *__restrict__ usedv) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t > ntris) return;
    if (t == ntris) {
        keep[t] = 0u; // ntris + 1 entries: the scan leaves the total in the last one
        return;
    }
    const uint32_t a = (uint32_t)faces[3 * t], b = (uint32_t)faces[3 * t + 1], c = (uint32_t)faces[3 * t + 2];
    if ((int64_t)a >= nverts || (int64_t)b >= nverts || (int64_t)c >= nverts) { // (never from this library's meshes)
        keep[t] = 0u;
        return;
    }
    const bool fa = (flags[a] != 0) != (invert != 0), fb = (flags[b] != 0) != (invert != 0), fc = (flags[c] != 0) != (invert != 0);
    const bool k = fa || fb || fc;
    keep[t] = k ? 1u : 0u;
    if (k) {
        usedv[a] = 1u;
        usedv[b] = 1u;
        usedv[c] = 1u;
    }
}

static inline size_t al256(size_t x) { return (x + 255) & ~(size_t)255; }
constexpr int BOUNDS_BLOCKS = 1024;

// per-stream WS_MESH2: [depth: width * height words][queue: ntris words][counter]
struct VisLayout {
    size_t off_queue, off_count, total;
};
static VisLayout vis_layout(int64_t npix, int64_t ntris) {
    VisLayout m;
    m.off_queue = al256((size_t)npix * 4);
    m.off_count = m.off_queue + al256((size_t)ntris * 4 + 4);
    m.total = m.off_count + 256;
    return m;
}

static int check_view(const ivx_mesh_view *v) {
    IVX_REQUIRE(v != nullptr, IVX_EINVAL, "mesh view: null");
    IVX_REQUIRE(v->width > 0 && v->height > 0 && (int64_t)v->width * v->height < 0x7fffffffll, IVX_EINVAL,
                "mesh view: viewport %d x %d", v->width, v->height);
    IVX_REQUIRE(v->zfar > v->znear && v->tan_half > 0.0 && v->aspect > 0.0, IVX_EINVAL, "mesh view: clipping range / angle / aspect");
    return IVX_OK;
}

// the three stages of one view into `depth` (device, width * height words); `queue` / `count` from the caller's workspace
static int raster_stages(const float *verts, int64_t nverts, const int32_t *faces, int64_t ntris, const ivx_mesh_view &V, int stages,
                         uint32_t *depth, uint32_t *queue, uint32_t *count, hipStream_t st) {
    if (stages & IVX_RASTER_CLEAR) {
        IVX_HIP(hipMemsetD32Async((hipDeviceptr_t)depth, (int)DEPTH_ONE, (size_t)V.width * V.height, st));
        IVX_HIP(hipMemsetAsync(count, 0, 4, st));
    }
    if (ntris == 0) return IVX_OK; // (no launch with an empty grid)
    if (stages & IVX_RASTER_SMALL) {
        hipLaunchKernelGGL(k_vis_raster_small, dim3((unsigned)ivx::cdiv(ntris, 256)), dim3(256), 0, st, verts, nverts, faces, ntris, V,
                           depth, queue, count);
        IVX_LAUNCH_CHECK();
    }
    if (stages & IVX_RASTER_BIG) {
        hipLaunchKernelGGL(k_vis_raster_big, dim3((unsigned)std::min<int64_t>(ntris, 2048)), dim3(256), 0, st, verts, nverts, faces, ntris,
                           V, depth, queue, count);
        IVX_LAUNCH_CHECK();
    }
    return IVX_OK;
}

static int check_mesh_sizes(int64_t nverts, int64_t ntris) {
    IVX_REQUIRE(nverts >= 0 && ntris >= 0, IVX_EINVAL, "mesh: negative size");
    IVX_REQUIRE(nverts < 0x7fffffffll && ntris < 0x7fffffffll, IVX_EINVAL, "mesh: more than 2^31 vertices / triangles");
    return IVX_OK;
}
static int check_faces(const int32_t *faces, int64_t ntris, int64_t nverts) {
    for (int64_t q = 0; q < 3 * ntris; q++)
        IVX_REQUIRE(faces[q] >= 0 && faces[q] < nverts, IVX_EDOM, "mesh: face index %d outside [0, %lld)", faces[q], (long long)nverts);
    return IVX_OK;
}

} // namespace

extern "C" int ivx_dev_mesh_bounds(const float *verts, int64_t nverts, float *bounds6, void *stream) {
    int rc;
    if ((rc = check_mesh_sizes(nverts, 0))) return rc;
    hipStream_t st = ivx::S(stream);
    if (nverts == 0) {
        IVX_HIP(hipMemsetAsync(bounds6, 0, 6 * sizeof(float), st));
        return IVX_OK;
    }
    const int nb = (int)std::min<int64_t>(ivx::cdiv(nverts, 256), BOUNDS_BLOCKS);
    void *ws;
    if ((rc = ivx::ws_get_s(ivx::WS_MESH, st, (size_t)BOUNDS_BLOCKS * 6 * 4, &ws))) return rc;
    hipLaunchKernelGGL(k_vis_bounds, dim3((unsigned)nb), dim3(256), 0, st, verts, nverts, (float *)ws);
    IVX_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_vis_bounds_final, dim3(1), dim3(256), 0, st, (const float *)ws, nb, bounds6);
    IVX_LAUNCH_CHECK();
    return IVX_OK;
}

extern "C" int ivx_dev_mesh_depth_raster(const float *verts, int64_t nverts, const int32_t *faces, int64_t ntris,
                                         const ivx_mesh_view *view, int stages, float *depth, void *stream) {
    int rc;
    if ((rc = check_mesh_sizes(nverts, ntris)) || (rc = check_view(view))) return rc;
    IVX_REQUIRE(stages > 0 && stages <= IVX_RASTER_ALL, IVX_EINVAL, "mesh raster: stages %d", stages);
    hipStream_t st = ivx::S(stream);
    const VisLayout m = vis_layout(0, ntris);
    void *ws;
    if ((rc = ivx::ws_get_s(ivx::WS_MESH2, st, m.total, &ws))) return rc;
    char *w = (char *)ws;
    return raster_stages(verts, nverts, faces, ntris, *view, stages, (uint32_t *)depth, (uint32_t *)(w + m.off_queue),
                         (uint32_t *)(w + m.off_count), st);
}

extern "C" int ivx_dev_mesh_visible_points(const float *verts, int64_t nverts, const int32_t *faces, int64_t ntris,
                                           const ivx_mesh_view *views, int nviews, uint8_t *flags, void *stream) {
    int rc;
    if ((rc = check_mesh_sizes(nverts, ntris))) return rc;
    IVX_REQUIRE(nviews >= 0, IVX_EINVAL, "mesh views: negative count");
    int64_t npix = 0;
    for (int q = 0; q < nviews; q++) {
        if ((rc = check_view(views + q))) return rc;
        npix = std::max<int64_t>(npix, (int64_t)views[q].width * views[q].height);
    }
    if (nverts == 0) return IVX_OK;
    hipStream_t st = ivx::S(stream);
    IVX_HIP(hipMemsetAsync(flags, 0, (size_t)nverts, st));
    if (nviews == 0) return IVX_OK;
    const VisLayout m = vis_layout(npix, ntris);
    void *ws;
    if ((rc = ivx::ws_get_s(ivx::WS_MESH2, st, m.total, &ws))) return rc;
    char *w = (char *)ws;
    uint32_t *depth = (uint32_t *)w, *queue = (uint32_t *)(w + m.off_queue), *count = (uint32_t *)(w + m.off_count);
    for (int q = 0; q < nviews; q++) {
        if ((rc = raster_stages(verts, nverts, faces, ntris, views[q], IVX_RASTER_ALL, depth, queue, count, st))) return rc;
        hipLaunchKernelGGL(k_vis_points, dim3((unsigned)ivx::cdiv(nverts, 256)), dim3(256), 0, st, verts, nverts, views[q],
                           (const float *)depth, flags);
        IVX_LAUNCH_CHECK();
    }
    return IVX_OK;
}

extern "C" int ivx_dev_mesh_select_points(const float *verts, int64_t nverts, const int32_t *faces, int64_t ntris,
                                          const uint8_t *flags, int invert, float *out_verts, int64_t max_verts, int32_t *out_faces,
                                          int64_t max_tris, int64_t *out_nverts, int64_t *out_ntris, void *stream) {
    int rc;
    if ((rc = check_mesh_sizes(nverts, ntris))) return rc;
    *out_nverts = 0;
    *out_ntris = 0;
    if (ntris == 0) return IVX_OK;
    hipStream_t st = ivx::S(stream);
    const size_t v4 = al256(((size_t)nverts + 1) * 4), t4 = al256(((size_t)ntris + 1) * 4);
    const size_t off_bsum = v4 + t4;
    const size_t off_misc = off_bsum + al256(((size_t)scan_u32_blocks(std::max(nverts, ntris) + 1) + 16) * 4);
    void *ws;
    if ((rc = ivx::ws_get_s(ivx::WS_MESH, st, off_misc + 256, &ws))) return rc;
    char *w = (char *)ws;
    uint32_t *usedv = (uint32_t *)w, *keep = (uint32_t *)(w + v4), *bsum = (uint32_t *)(w + off_bsum);
    uint32_t *tot_t = (uint32_t *)(w + off_misc), *tot_v = tot_t + 1;
    IVX_HIP(hipMemsetAsync(usedv, 0, ((size_t)nverts + 1) * 4, st));
    hipLaunchKernelGGL(k_vis_mark, dim3((unsigned)ivx::cdiv(ntris + 1, 256)), dim3(256), 0, st, faces, ntris, nverts, flags, invert,
                       keep, usedv);
    IVX_LAUNCH_CHECK();
    if ((rc = scan_u32_exclusive(keep, ntris + 1, bsum, tot_t, st))) return rc;
    if ((rc = scan_u32_exclusive(usedv, nverts + 1, bsum, tot_v, st))) return rc;
    uint32_t seq, got[2];
    if ((rc = ivx::mailbox_publish(tot_t, 2, st, &seq))) return rc;
    if ((rc = ivx::mailbox_wait(seq, st, got, 2))) return rc;
    *out_ntris = got[0];
    *out_nverts = got[1];
    if (!out_verts || !out_faces || got[0] == 0) return IVX_OK;
    IVX_REQUIRE(max_tris >= (int64_t)got[0] && max_verts >= (int64_t)got[1], IVX_ERANGE,
                "mesh: output buffers too small (%u verts, %u triangles needed)", got[1], got[0]);
    hipLaunchKernelGGL(k_mesh_compact_faces, dim3((unsigned)ivx::cdiv(ntris, 256)), dim3(256), 0, st, faces, ntris, keep, usedv,
                       out_faces, max_tris);
    IVX_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_mesh_compact_verts, dim3((unsigned)ivx::cdiv(nverts, 256)), dim3(256), 0, st, verts, nverts, usedv,
                       out_verts, max_verts);
    IVX_LAUNCH_CHECK();
    return IVX_OK;
}

// ---- host forms -----------------------------------------------------------------------------------------------------
namespace {
// the mesh into WS_IN (points) / WS_AUX0 (triangles)
int upload_mesh(const float *verts, int64_t nverts, const int32_t *faces, int64_t ntris, void **d_v, void **d_f) {
    using namespace ivx;
    int rc;
    if ((rc = check_mesh_sizes(nverts, ntris)) || (rc = check_faces(faces, ntris, nverts))) return rc;
    if ((rc = ws_get(WS_IN, (size_t)nverts * 12 + 16, d_v))) return rc;
    if ((rc = ws_get(WS_AUX0, (size_t)ntris * 12 + 16, d_f))) return rc;
    if (nverts) IVX_HIP(hipMemcpy(*d_v, verts, (size_t)nverts * 12, hipMemcpyHostToDevice));
    if (ntris) IVX_HIP(hipMemcpy(*d_f, faces, (size_t)ntris * 12, hipMemcpyHostToDevice));
    return IVX_OK;
}
// flags (device, WS_AUX2) -> the selection on the uploaded mesh -> host arrays
int select_to_host(const void *d_v, int64_t nverts, const void *d_f, int64_t ntris, const void *d_flags, int invert, float *out_verts,
                   int32_t *out_faces, int64_t *out_nverts, int64_t *out_ntris) {
    using namespace ivx;
    void *d_ov = nullptr, *d_of = nullptr;
    int rc;
    const bool fill = out_verts && out_faces;
    if (fill) {
        if ((rc = ws_get(WS_OUT, (size_t)nverts * 12 + 16, &d_ov))) return rc;
        if ((rc = ws_get(WS_AUX1, (size_t)ntris * 12 + 16, &d_of))) return rc;
    }
    if ((rc = ivx_dev_mesh_select_points((const float *)d_v, nverts, (const int32_t *)d_f, ntris, (const uint8_t *)d_flags, invert,
                                         (float *)d_ov, nverts, (int32_t *)d_of, ntris, out_nverts, out_ntris, nullptr)))
        return rc;
    IVX_HIP(hipDeviceSynchronize());
    if (fill && *out_nverts) IVX_HIP(hipMemcpy(out_verts, d_ov, (size_t)*out_nverts * 12, hipMemcpyDeviceToHost));
    if (fill && *out_ntris) IVX_HIP(hipMemcpy(out_faces, d_of, (size_t)*out_ntris * 12, hipMemcpyDeviceToHost));
    return IVX_OK;
}
} // namespace

extern "C" int ivx_mesh_bounds(const float *verts, int64_t nverts, float *bounds6) {
    ivx::HostCallGuard host_guard__;
    using namespace ivx;
    int rc;
    if ((rc = check_mesh_sizes(nverts, 0))) return rc;
    for (int q = 0; q < 6; q++) bounds6[q] = 0.0f;
    if (nverts == 0) return IVX_OK;
    void *d_v, *d_o;
    if ((rc = ws_get(WS_IN, (size_t)nverts * 12 + 16, &d_v))) return rc;
    if ((rc = ws_get(WS_SMALL, 64, &d_o))) return rc;
    IVX_HIP(hipMemcpy(d_v, verts, (size_t)nverts * 12, hipMemcpyHostToDevice));
    if ((rc = ivx_dev_mesh_bounds((const float *)d_v, nverts, (float *)d_o, nullptr))) return rc;
    IVX_HIP(hipMemcpy(bounds6, d_o, 6 * sizeof(float), hipMemcpyDeviceToHost));
    return IVX_OK;
}

extern "C" int ivx_mesh_depth_raster(const float *verts, int64_t nverts, const int32_t *faces, int64_t ntris,
                                     const ivx_mesh_view *view, float *depth) {
    ivx::HostCallGuard host_guard__;
    using namespace ivx;
    int rc;
    if ((rc = check_view(view))) return rc;
    void *d_v, *d_f, *d_z;
    if ((rc = upload_mesh(verts, nverts, faces, ntris, &d_v, &d_f))) return rc;
    const size_t nz = (size_t)view->width * view->height * 4;
    if ((rc = ws_get(WS_OUT, nz, &d_z))) return rc;
    if ((rc = ivx_dev_mesh_depth_raster((const float *)d_v, nverts, (const int32_t *)d_f, ntris, view, IVX_RASTER_ALL, (float *)d_z,
                                        nullptr)))
        return rc;
    IVX_HIP(hipMemcpy(depth, d_z, nz, hipMemcpyDeviceToHost));
    return IVX_OK;
}

extern "C" int ivx_mesh_visible_points(const float *verts, int64_t nverts, const int32_t *faces, int64_t ntris,
                                       const ivx_mesh_view *views, int nviews, uint8_t *flags) {
    ivx::HostCallGuard host_guard__;
    using namespace ivx;
    int rc;
    void *d_v, *d_f, *d_fl;
    if ((rc = upload_mesh(verts, nverts, faces, ntris, &d_v, &d_f))) return rc;
    if ((rc = ws_get(WS_AUX2, (size_t)nverts + 16, &d_fl))) return rc;
    if ((rc = ivx_dev_mesh_visible_points((const float *)d_v, nverts, (const int32_t *)d_f, ntris, views, nviews, (uint8_t *)d_fl,
                                          nullptr)))
        return rc;
    if (nverts) IVX_HIP(hipMemcpy(flags, d_fl, (size_t)nverts, hipMemcpyDeviceToHost));
    return IVX_OK;
}

extern "C" int ivx_mesh_select_points(const float *verts, int64_t nverts, const int32_t *faces, int64_t ntris, const uint8_t *flags,
                                      int invert, float *out_verts, int32_t *out_faces, int64_t *out_nverts, int64_t *out_ntris) {
    ivx::HostCallGuard host_guard__;
    using namespace ivx;
    int rc;
    *out_nverts = *out_ntris = 0;
    void *d_v, *d_f, *d_fl;
    if ((rc = upload_mesh(verts, nverts, faces, ntris, &d_v, &d_f))) return rc;
    if (ntris == 0) return IVX_OK;
    if ((rc = ws_get(WS_AUX2, (size_t)nverts + 16, &d_fl))) return rc;
    IVX_HIP(hipMemcpy(d_fl, flags, (size_t)nverts, hipMemcpyHostToDevice));
    return select_to_host(d_v, nverts, d_f, ntris, d_fl, invert, out_verts, out_faces, out_nverts, out_ntris);
}

extern "C" int ivx_mesh_remove_nonvisible(const float *verts, int64_t nverts, const int32_t *faces, int64_t ntris,
                                          const ivx_mesh_view *views, int nviews, int remove_visible, float *out_verts,
                                          int32_t *out_faces, int64_t *out_nverts, int64_t *out_ntris) {
    ivx::HostCallGuard host_guard__;
    using namespace ivx;
    int rc;
    *out_nverts = *out_ntris = 0;
    void *d_v, *d_f, *d_fl;
    if ((rc = upload_mesh(verts, nverts, faces, ntris, &d_v, &d_f))) return rc;
    if (nverts == 0) return IVX_OK;
    if ((rc = ws_get(WS_AUX2, (size_t)nverts + 16, &d_fl))) return rc;
    if ((rc = ivx_dev_mesh_visible_points((const float *)d_v, nverts, (const int32_t *)d_f, ntris, views, nviews, (uint8_t *)d_fl,
                                          nullptr)))
        return rc;
    if (ntris == 0) return IVX_OK;
    return select_to_host(d_v, nverts, d_f, ntris, d_fl, remove_visible, out_verts, out_faces, out_nverts, out_ntris);
}
