// k_slice_show.hip -- the slice display: Slice.GetSlices (invesalius/data/slice_.py:746-830) as one launch.
//
// Reference chain: do_ww_wl -> do_colour_image -> do_colour_mask + do_blend -> do_custom_colour + do_blend.  VTK is not
// available to this project, so the arithmetic of its filters is stated as rules R1 - R7 in slice_show_math.h and in
// tests/_slice_display_ref.py; the kernel is held to that statement bit for bit (DESIGN 7l says what is unpinned).
//
// MI355X design: per pixel 2 B of image, 1 B of mask and 1 B of aux come in and 3 B go out, so a 512 x 512 picture moves 1.8 MB
// and is bound by the launch, not by HBM.  One launch per picture.  The three 256-entry RGBA tables (image, mask, aux) and the
// widget's nodes are copied to LDS by every workgroup (3 KB + 32 B per node).  A lane takes four neighbouring pixels of a row:
// one 8-byte image load where the row's element stride is 2 and the address is 8-byte aligned, one dword of mask and of aux
// where those are contiguous and aligned, three dword stores of RGB where the row's first output byte is 4-byte aligned.  The
// tail of a row, unaligned rows and strided views (a sagittal slice of a resident volume: the element stride is the volume's
// row pitch) take the same arithmetic through scalar loads and byte stores.  Every load and store is guarded by y < h, x < w;
// every table index is clamped by slice_show_math.h.
#include "ivx_internal.h"
#include "slice_show_math.h"

namespace ss = ivx_slice_show_math;

namespace {

struct ShowArgs {
    const uint8_t *img;
    int64_t irs, ies;
    const uint8_t *mask;
    int64_t mrs, mes;
    const uint8_t *aux;
    int64_t ars, aes;
    uint8_t *out;
    const uint8_t *tables; // 3 x 256 RGBA, then n_nodes values and 3 n_nodes colours (float64)
    int64_t h, w;
    int kind, mode, stages, n_nodes, och;
    ss::Window W;
};

__device__ inline uint32_t blend(uint32_t c, uint32_t over) {
    const int a = (int)(over >> 24);
    const uint32_t r = (uint32_t)ss::r7_blend((int)(c & 255), (int)(over & 255), a);
    const uint32_t g = (uint32_t)ss::r7_blend((int)((c >> 8) & 255), (int)((over >> 8) & 255), a);
    const uint32_t b = (uint32_t)ss::r7_blend((int)((c >> 16) & 255), (int)((over >> 16) & 255), a);
    return r | (g << 8) | (b << 16);
}

// one pixel: `v` the image value (or the grey byte), `rgb` the picture's pixel for IMG_RGB8, `m` / `x` the mask's and aux's
// byte (or their RGBA pixel when the stage that colours them is off)
__device__ inline uint32_t shade(const ShowArgs &a, const uint32_t *tab, const double *nv, const double *nc, double v, uint32_t rgb,
                                 uint32_t m, uint32_t x) {
    uint32_t c;
    if (a.kind == ss::IMG_RGB8)
        c = rgb;
    else if (!(a.stages & ss::ST_WWWL))
        c = (uint32_t)ss::u8(v) * 0x010101u;
    else if (a.mode == ss::MODE_PLIST)
        c = tab[ss::r3_index(a.W, v)] & 0xffffffu;
    else if (a.mode == ss::MODE_WIDGET) {
        int o[3];
        ss::r4_colour(nv, nc, a.n_nodes, v, o);
        c = (uint32_t)o[0] | ((uint32_t)o[1] << 8) | ((uint32_t)o[2] << 16);
    } else
        c = (uint32_t)ss::r1_grey(a.W, v) * 0x010101u;
    if ((a.stages & ss::ST_COLOUR) && a.mode == ss::MODE_OTHER) c = tab[ss::r2_index(a.W, (int)(c & 255))] & 0xffffffu;
    uint32_t over = 0;
    if (a.mask) {
        over = (a.stages & ss::ST_MASK) ? tab[256 + (m & 255)] : m;
        if (a.stages & ss::ST_BLEND) c = blend(c, over);
    }
    if (a.aux) {
        const uint32_t o2 = (a.stages & ss::ST_AUX) ? tab[512 + ss::r6_index(a.W, (int)(x & 255))] : x;
        if (a.stages & ss::ST_BLEND) c = blend(c, o2);
        else if (!a.mask)
            over = o2;
    }
    return a.och == 4 ? over : c;
}

__device__ inline uint32_t load_rgba(const uint8_t *p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }

// an overlay operand's four pixels: bytes to be coloured (one dword where contiguous and aligned), or RGBA pixels
__device__ inline void load_overlay(const uint8_t *base, int64_t rs, int64_t es, bool coloured, int64_t y, int64_t x0, int cnt, uint32_t o[4]) {
    o[0] = o[1] = o[2] = o[3] = 0;
    if (!base) return;
    const uint8_t *p = base + y * rs + x0 * es;
    if (!coloured) {
#pragma unroll
        for (int k = 0; k < 4; k++)
            if (k < cnt) o[k] = load_rgba(p + k * es);
    } else if (cnt == 4 && es == 1 && (((uintptr_t)p) & 3) == 0) {
        const uint32_t q = *reinterpret_cast<const uint32_t *>(p);
        o[0] = q & 255, o[1] = (q >> 8) & 255, o[2] = (q >> 16) & 255, o[3] = q >> 24;
    } else {
#pragma unroll
        for (int k = 0; k < 4; k++)
            if (k < cnt) o[k] = p[k * es];
    }
}

__global__ __launch_bounds__(256) void k_slice_show(const ShowArgs a) {
    __shared__ uint32_t tab[768];
    __shared__ double nv[ss::MAX_NODES];
    __shared__ double nc[3 * ss::MAX_NODES];
    {
        const uint32_t *t = reinterpret_cast<const uint32_t *>(a.tables);
        for (int i = threadIdx.x; i < 768; i += 256) tab[i] = t[i];
        const double *d = reinterpret_cast<const double *>(a.tables + 3072);
        for (int i = threadIdx.x; i < a.n_nodes; i += 256) nv[i] = d[i];
        for (int i = threadIdx.x; i < 3 * a.n_nodes; i += 256) nc[i] = d[a.n_nodes + i];
    }
    __syncthreads();
    const int64_t per_row = (a.w + 3) / 4;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.h * per_row) return;
    const int64_t y = i / per_row, x0 = (i - y * per_row) * 4;
    const int cnt = a.w - x0 < 4 ? (int)(a.w - x0) : 4;

    double v[4] = {0.0, 0.0, 0.0, 0.0};
    uint32_t rgb[4] = {0, 0, 0, 0};
    if (a.img) {
        const uint8_t *p = a.img + y * a.irs + x0 * a.ies;
        if (a.kind == ss::IMG_I16) {
            if (cnt == 4 && a.ies == 2 && (((uintptr_t)p) & 7) == 0) {
                const uint2 q = *reinterpret_cast<const uint2 *>(p);
                v[0] = (double)(int16_t)(q.x & 0xffffu), v[1] = (double)(int16_t)(q.x >> 16);
                v[2] = (double)(int16_t)(q.y & 0xffffu), v[3] = (double)(int16_t)(q.y >> 16);
            } else {
#pragma unroll
                for (int k = 0; k < 4; k++)
                    if (k < cnt) v[k] = (double)*reinterpret_cast<const int16_t *>(p + k * a.ies);
            }
        } else if (a.kind == ss::IMG_F64) {
#pragma unroll
            for (int k = 0; k < 4; k++)
                if (k < cnt) v[k] = *reinterpret_cast<const double *>(p + k * a.ies);
        } else if (a.kind == ss::IMG_U8) {
#pragma unroll
            for (int k = 0; k < 4; k++)
                if (k < cnt) v[k] = (double)p[k * a.ies];
        } else {
#pragma unroll
            for (int k = 0; k < 4; k++)
                if (k < cnt) {
                    const uint8_t *q = p + k * a.ies;
                    rgb[k] = (uint32_t)q[0] | ((uint32_t)q[1] << 8) | ((uint32_t)q[2] << 16);
                }
        }
    }
    uint32_t m[4], x[4];
    load_overlay(a.mask, a.mrs, a.mes, (a.stages & ss::ST_MASK) != 0, y, x0, cnt, m);
    load_overlay(a.aux, a.ars, a.aes, (a.stages & ss::ST_AUX) != 0, y, x0, cnt, x);

    uint32_t c[4] = {0, 0, 0, 0};
#pragma unroll
    for (int k = 0; k < 4; k++)
        if (k < cnt) c[k] = shade(a, tab, nv, nc, v[k], rgb[k], m[k], x[k]);

    const int64_t pix = y * a.w + x0;
    if (a.och == 4) { // RGBA of an overlay alone: the block is 4-byte aligned (checked by the host)
        uint32_t *o = reinterpret_cast<uint32_t *>(a.out) + pix;
#pragma unroll
        for (int k = 0; k < 4; k++)
            if (k < cnt) o[k] = c[k];
        return;
    }
    uint8_t *o = a.out + pix * 3;
    if (cnt == 4 && (((uintptr_t)o) & 3) == 0) {
        uint32_t *o4 = reinterpret_cast<uint32_t *>(o);
        o4[0] = c[0] | (c[1] << 24);
        o4[1] = (c[1] >> 8) | (c[2] << 16);
        o4[2] = (c[2] >> 16) | (c[3] << 8);
    } else {
#pragma unroll
        for (int k = 0; k < 4; k++)
            if (k < cnt) {
                o[3 * k] = (uint8_t)(c[k] & 255);
                o[3 * k + 1] = (uint8_t)((c[k] >> 8) & 255);
                o[3 * k + 2] = (uint8_t)((c[k] >> 16) & 255);
            }
    }
}

static size_t image_item(int kind) { return kind == ss::IMG_I16 ? 2 : (kind == ss::IMG_F64 ? 8 : 1); }

static int check_params(const ivx_slice_show_params *p, bool image, bool mask, bool aux) {
    IVX_REQUIRE(p, IVX_EINVAL, "slice_show: no parameter block");
    IVX_REQUIRE(p->image_kind >= ss::IMG_I16 && p->image_kind <= ss::IMG_RGB8, IVX_EINVAL, "slice_show: image kind %d", p->image_kind);
    IVX_REQUIRE(p->mode >= ss::MODE_OTHER && p->mode <= ss::MODE_WIDGET, IVX_EINVAL, "slice_show: colour mode %d", p->mode);
    IVX_REQUIRE((p->stages & ~ss::ST_ALL) == 0, IVX_EINVAL, "slice_show: unknown stage bits %d", p->stages);
    IVX_REQUIRE(p->n_nodes >= 0 && p->n_nodes <= ss::MAX_NODES, IVX_EINVAL, "slice_show: %d widget nodes (at most %d)", p->n_nodes, (int)ss::MAX_NODES);
    IVX_REQUIRE(p->aux_max >= 0 && p->aux_max <= 255, IVX_EINVAL, "slice_show: largest aux key %d", p->aux_max);
    IVX_REQUIRE(p->out_channels == 3 || p->out_channels == 4, IVX_EINVAL, "slice_show: %d output channels", p->out_channels);
    if (p->out_channels == 3) {
        IVX_REQUIRE(image, IVX_EINVAL, "slice_show: an RGB picture needs the image operand");
        const bool raw = p->image_kind == ss::IMG_I16 || p->image_kind == ss::IMG_F64;
        IVX_REQUIRE(raw == ((p->stages & ss::ST_WWWL) != 0), IVX_EINVAL,
                    "slice_show: the window/level stage takes int16 or float64 values, every other stage a picture's bytes");
        if (p->stages & ss::ST_WWWL) {
            IVX_REQUIRE(p->window_width > 0.0, IVX_EDOM, "slice_show: window width %g", p->window_width);
            IVX_REQUIRE(p->mode != ss::MODE_WIDGET || p->n_nodes >= 1, IVX_EINVAL, "slice_show: the widget mode needs nodes");
        }
    } else
        IVX_REQUIRE(!(p->stages & ss::ST_BLEND) && (mask != aux), IVX_EINVAL, "slice_show: an RGBA picture is one overlay, not blended");
    return IVX_OK;
}

} // namespace

static size_t tables_bytes(int n_nodes) { return 3072 + (size_t)n_nodes * 32; }

extern "C" int ivx_slice_show_tables_bytes(int n_nodes, size_t *nbytes) {
    IVX_REQUIRE(nbytes && n_nodes >= 0 && n_nodes <= ss::MAX_NODES, IVX_EINVAL, "slice_show_tables_bytes: %d nodes", n_nodes);
    *nbytes = tables_bytes(n_nodes);
    return IVX_OK;
}

extern "C" int ivx_dev_slice_show(const void *image, int64_t image_row_stride, int64_t image_elem_stride, const uint8_t *mask,
                                  int64_t mask_row_stride, int64_t mask_elem_stride, const uint8_t *aux, int64_t aux_row_stride,
                                  int64_t aux_elem_stride, int64_t h, int64_t w, const ivx_slice_show_params *p, const void *tables,
                                  uint8_t *out, void *stream) {
    IVX_REQUIRE(h >= 0 && w >= 0, IVX_EINVAL, "slice_show: negative size");
    int rc;
    if ((rc = check_params(p, image != nullptr, mask != nullptr, aux != nullptr))) return rc;
    IVX_REQUIRE(tables && out, IVX_EINVAL, "slice_show: tables and output are required");
    IVX_REQUIRE((((uintptr_t)tables) & 7) == 0, IVX_EINVAL, "slice_show: the tables block is not 8-byte aligned");
    const size_t isz = image_item(p->image_kind);
    IVX_REQUIRE(!image || ((((uintptr_t)image) | (uintptr_t)image_row_stride | (uintptr_t)image_elem_stride) & (isz - 1)) == 0, IVX_EINVAL,
                "slice_show: the image view is not aligned to its elements");
    IVX_REQUIRE(p->out_channels == 3 || (((uintptr_t)out) & 3) == 0, IVX_EINVAL, "slice_show: the RGBA output is not 4-byte aligned");
    if (h == 0 || w == 0) return IVX_OK;
    const int64_t lanes = h * ((w + 3) / 4);
    const int64_t blocks = ivx::cdiv(lanes, 256);
    IVX_REQUIRE(blocks < ((int64_t)1 << 31), IVX_EINVAL, "slice_show: %lld workgroups", (long long)blocks);
    ShowArgs a;
    a.img = (const uint8_t *)image, a.irs = image_row_stride, a.ies = image_elem_stride;
    a.mask = mask, a.mrs = mask_row_stride, a.mes = mask_elem_stride;
    a.aux = aux, a.ars = aux_row_stride, a.aes = aux_elem_stride;
    a.out = out, a.tables = (const uint8_t *)tables, a.h = h, a.w = w;
    a.kind = p->image_kind, a.mode = p->mode, a.stages = p->stages, a.n_nodes = p->n_nodes, a.och = p->out_channels;
    a.W = ss::make_window(p->window_width, p->window_level, p->image_kind == ss::IMG_F64, p->table_min, p->table_max, p->aux_max);
    hipLaunchKernelGGL(k_slice_show, dim3((unsigned)blocks), dim3(256), 0, ivx::S(stream), a);
    IVX_LAUNCH_CHECK();
    return IVX_OK;
}

// host form: the three views are staged dense -- from the mirror when their array is registered (no byte crosses the link),
// else the slice alone is uploaded -- and the picture comes back in one copy
extern "C" int ivx_slice_show(const void *image, int64_t image_row_stride, int64_t image_elem_stride, const uint8_t *mask,
                              int64_t mask_row_stride, int64_t mask_elem_stride, const uint8_t *aux, int64_t aux_row_stride,
                              int64_t aux_elem_stride, int64_t h, int64_t w, const ivx_slice_show_params *p, const void *tables,
                              uint8_t *out) {
    ivx::HostCallGuard host_guard__;
    using namespace ivx;
    IVX_REQUIRE(h >= 0 && w >= 0, IVX_EINVAL, "slice_show: negative size");
    int rc;
    if ((rc = check_params(p, image != nullptr, mask != nullptr, aux != nullptr))) return rc;
    IVX_REQUIRE(tables && out, IVX_EINVAL, "slice_show: tables and output are required");
    const size_t npix = (size_t)h * w;
    if (npix == 0) return IVX_OK;
    // a view of k-byte pixels as a (h, w, k) box of bytes, or as (1, h, w) items
    auto stage = [&](int slot, const void *src, int64_t rs, int64_t es, size_t item, int64_t bytes_per_pixel, void **d) -> int {
        int r;
        if ((r = ws_get(slot, npix * item * bytes_per_pixel + 16, d))) return r;
        if (bytes_per_pixel == 1) {
            const int64_t sh[3] = {1, h, w}, st[3] = {rs * h, rs, es};
            return upload_strided(*d, src, sh, st, item, slot);
        }
        const int64_t sh[3] = {h, w, bytes_per_pixel}, st[3] = {rs, es, 1};
        return upload_strided(*d, src, sh, st, 1, slot);
    };
    void *d_i = nullptr, *d_m = nullptr, *d_a = nullptr, *d_t, *d_o;
    const size_t isz = image_item(p->image_kind);
    const int64_t ipx = p->image_kind == ss::IMG_RGB8 ? 3 : 1;
    if (image && (rc = stage(WS_IN, image, image_row_stride, image_elem_stride, isz, ipx, &d_i))) return rc;
    const int64_t mpx = (p->stages & ss::ST_MASK) ? 1 : 4, apx = (p->stages & ss::ST_AUX) ? 1 : 4;
    if (mask && (rc = stage(WS_AUX0, mask, mask_row_stride, mask_elem_stride, 1, mpx, &d_m))) return rc;
    if (aux && (rc = stage(WS_AUX1, aux, aux_row_stride, aux_elem_stride, 1, apx, &d_a))) return rc;
    const size_t tb = tables_bytes(p->n_nodes);
    if ((rc = ws_get(WS_SMALL, tb, &d_t))) return rc;
    if ((rc = copy_h2d(d_t, tables, tb))) return rc;
    const size_t ob = npix * (size_t)p->out_channels;
    if ((rc = ws_get(WS_OUT, ob, &d_o))) return rc;
    if ((rc = ivx_dev_slice_show(d_i, w * (int64_t)isz * ipx, (int64_t)isz * ipx, (const uint8_t *)d_m, w * mpx, mpx, (const uint8_t *)d_a,
                                 w * apx, apx, h, w, p, d_t, (uint8_t *)d_o, nullptr)))
        return rc;
    IVX_HIP(hipDeviceSynchronize());
    return copy_d2h(out, d_o, ob);
}
