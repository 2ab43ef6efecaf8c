// k_slice_edit.hip -- the slice editing tools: the brush stroke of the manual edition panel and crop mask.
//
// Reference semantics (byte-exact):
//   brush stroke  Slice.edit_mask_pixel (invesalius/data/slice_.py:656-744), the watershed marker brush and the generic
//                 fill-value brush (styles.py:2000-2069, :392-461): one operation's value written under a footprint
//   crop mask     CropMaskInteractorStyle.CropMask (styles.py:2654-2694): everything outside a box becomes 1
//
// MI355X design: a stroke writes a few thousand bytes of one slice, so the cost is the launch, not the bytes.  A whole drag
// of one operation is ONE launch: workgroup (tile, dab) takes 256 consecutive footprint pixels of one dab and stores the
// operation's value with plain byte stores.  Every operation's value depends only on the pixel (its image value), so dabs that
// overlap store identical bytes and the result equals the dabs applied one after another -- no atomics, no ordering between
// workgroups.  Consecutive lanes walk the footprint's row: the footprint reads are coalesced, and so are the stores wherever
// the view's element stride is 1 (axial, coronal, and the dense staging copy of the host form).  A sagittal view of a resident
// block has an element stride of one row pitch: each store is then its own 64-byte line, which at these sizes (at most
// 201 x 201 pixels per dab) stays far below one launch latency.  The arithmetic -- window, bounds test, address, value -- is
// slice_edit_math.h, shared with the host build the CPU tests run.
#include <algorithm>

#include "ivx_internal.h"
#include "slice_edit_math.h"

namespace se = ivx_slice_edit;

namespace {

__global__ __launch_bounds__(256) void k_brush_stroke(uint8_t *__restrict__ mask, int64_t mrs, int64_t mes,
                                                      const uint8_t *__restrict__ image, int64_t irs, int64_t ies, int64_t h,
                                                      int64_t w, const uint8_t *__restrict__ fp, int64_t fh, int64_t fw,
                                                      const int32_t *__restrict__ dabs, int64_t ndabs, int op, int lo, int hi,
                                                      int fill) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= fh * fw || !fp[p]) return;
    const int64_t fy = p / fw, fx = p - fy * fw;
    for (int64_t d = blockIdx.y; d < ndabs; d += gridDim.y) {
        int64_t y, x;
        if (!se::dab_pixel(dabs[2 * d], dabs[2 * d + 1], fy, fx, h, w, &y, &x)) continue; // inside the slice, whatever the host clipped
        int v = 0;
        if (image) v = *reinterpret_cast<const int16_t *>(image + se::view_offset(y, x, irs, ies));
        const int out = se::op_value(op, v, lo, hi, fill);
        if (out >= 0) mask[se::view_offset(y, x, mrs, mes)] = (uint8_t)out;
    }
}

// everything outside [z0, z1) x [y0, y1) x [x0, x1) becomes 1; 16 bytes per lane where the block is aligned
__global__ __launch_bounds__(256) void k_mask_crop(uint8_t *__restrict__ m, int64_t n, int64_t dy, int64_t dx, int64_t z0, int64_t z1,
                                                   int64_t y0, int64_t y1, int64_t x0, int64_t x1, int vec) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t per = vec ? 16 : 1;
    const int64_t at = i * per;
    if (at >= n) return;
    const int64_t len = n - at < per ? n - at : per;
    int64_t x = at % dx, r = at / dx, y = r % dy, z = r / dy;
    bool keep[16];
    bool any = false;
    for (int q = 0; q < 16; q++) {
        keep[q] = q < len && z >= z0 && z < z1 && y >= y0 && y < y1 && x >= x0 && x < x1;
        any |= keep[q];
        if (++x == dx) {
            x = 0;
            if (++y == dy) {
                y = 0;
                z++;
            }
        }
    }
    if (len == 16 && !any) {
        *reinterpret_cast<uint4 *>(m + at) = make_uint4(0x01010101u, 0x01010101u, 0x01010101u, 0x01010101u);
        return;
    }
    for (int q = 0; q < len; q++)
        if (!keep[q]) m[at + q] = 1;
}

struct SliceGeom {
    int64_t h, w;       // the slice, interior voxels
    int64_t mrs, mes;   // mask view: row / element stride (bytes)
    int64_t irs, ies;   // image view
    int64_t moff, ioff; // byte offsets of the views' first element
    int64_t flag_off;   // the slice's flag cell in the padded matrix
};
// the three views of Slice.get_mask_slice (slice_.py:1142-1173): padded mask matrix[n+1, 1:, 1:] and siblings, image[n] and siblings
static int slice_geom(const int64_t ishape[3], const int64_t mst[3], const int64_t ist[3], int orientation, int64_t n, SliceGeom *g) {
    const int ax = orientation, r = ax == 0 ? 1 : 0, e = ax == 2 ? 1 : 2;
    IVX_REQUIRE(ax >= 0 && ax <= 2, IVX_EINVAL, "slice edit: orientation must be 0 (AXIAL), 1 (CORONAL) or 2 (SAGITAL)");
    IVX_REQUIRE(ishape[0] >= 0 && ishape[1] >= 0 && ishape[2] >= 0, IVX_EINVAL, "slice edit: negative shape");
    IVX_REQUIRE(n >= 0 && n < ishape[ax], IVX_ERANGE, "slice edit: slice %lld outside 0 .. %lld", (long long)n, (long long)ishape[ax] - 1);
    g->h = ishape[r], g->w = ishape[e];
    g->mrs = mst[r], g->mes = mst[e];
    g->moff = (n + 1) * mst[ax] + mst[r] + mst[e];
    g->flag_off = (n + 1) * mst[ax];
    if (ist) {
        g->irs = ist[r], g->ies = ist[e];
        g->ioff = n * ist[ax];
    } else
        g->irs = g->ies = g->ioff = 0;
    return IVX_OK;
}

} // namespace

extern "C" int ivx_dev_mask_brush_stroke(uint8_t *mask, int64_t mask_row_stride, int64_t mask_elem_stride, const int16_t *image,
                                         int64_t image_row_stride, int64_t image_elem_stride, int64_t h, int64_t w,
                                         const uint8_t *footprint, int64_t fh, int64_t fw, const int32_t *dabs, int64_t ndabs,
                                         int operation, int thresh_min, int thresh_max, int fill_value, void *stream) {
    IVX_REQUIRE(h >= 0 && w >= 0 && fh >= 0 && fw >= 0 && ndabs >= 0, IVX_EINVAL, "brush_stroke: negative size");
    IVX_REQUIRE(operation >= se::OP_DRAW && operation <= se::OP_FILL, IVX_EINVAL, "brush_stroke: unknown operation %d", operation);
    IVX_REQUIRE(fh * fw < ((int64_t)1 << 31), IVX_EINVAL, "brush_stroke: footprint of %lld x %lld pixels", (long long)fh, (long long)fw);
    const bool reads = se::op_reads_image(operation);
    IVX_REQUIRE(!reads || image, IVX_EINVAL, "brush_stroke: operation %d reads the image", operation);
    IVX_REQUIRE(!reads || ((((uintptr_t)image) | (uintptr_t)image_row_stride | (uintptr_t)image_elem_stride) & 1) == 0, IVX_EINVAL,
                "brush_stroke: the image view is not aligned to its int16 elements");
    if (h == 0 || w == 0 || fh * fw == 0 || ndabs == 0) return IVX_OK;
    const dim3 grid((unsigned)ivx::cdiv(fh * fw, 256), (unsigned)std::min<int64_t>(ndabs, 4096));
    hipLaunchKernelGGL(k_brush_stroke, grid, dim3(256), 0, ivx::S(stream), mask, mask_row_stride, mask_elem_stride,
                       reads ? (const uint8_t *)image : nullptr, image_row_stride, image_elem_stride, h, w, footprint, fh, fw, dabs,
                       ndabs, operation, thresh_min, thresh_max, fill_value);
    IVX_LAUNCH_CHECK();
    return IVX_OK;
}

extern "C" int ivx_dev_mask_crop(uint8_t *mask, int64_t dz, int64_t dy, int64_t dx, const int64_t box[6], void *stream) {
    IVX_REQUIRE(dz >= 0 && dy >= 0 && dx >= 0, IVX_EINVAL, "mask_crop: negative shape");
    const int64_t n = dz * dy * dx;
    if (n == 0) return IVX_OK;
    const int vec = (((uintptr_t)mask) & 15) == 0;
    const int64_t blocks = ivx::cdiv(ivx::cdiv(n, vec ? 16 : 1), 256);
    IVX_REQUIRE(blocks < ((int64_t)1 << 31), IVX_EINVAL, "mask_crop: %lld workgroups", (long long)blocks);
    hipLaunchKernelGGL(k_mask_crop, dim3((unsigned)blocks), dim3(256), 0, ivx::S(stream), mask, n, dy, dx, box[0], box[1], box[2],
                       box[3], box[4], box[5], vec);
    IVX_LAUNCH_CHECK();
    return IVX_OK;
}

// ---- slice_edit_math.h for host callers (no device needed) ---------------------------------------------------------------------
extern "C" int ivx_slice_flat_position(int64_t position, int64_t slice_width, double out_xy[2]) {
    IVX_REQUIRE(slice_width > 0, IVX_EINVAL, "flat_position: slice width %lld", (long long)slice_width);
    se::flat_position(position, slice_width, &out_xy[0], &out_xy[1]);
    return IVX_OK;
}

extern "C" int ivx_slice_dab_windows(const double *positions_xy, int64_t ndabs, int64_t fh, int64_t fw, int32_t *dabs) {
    IVX_REQUIRE(ndabs >= 0 && fh >= 0 && fw >= 0, IVX_EINVAL, "dab_windows: negative size");
    for (int64_t k = 0; k < ndabs; k++) {
        dabs[2 * k] = (int32_t)se::window_start(positions_xy[2 * k], fw);
        dabs[2 * k + 1] = (int32_t)se::window_start(positions_xy[2 * k + 1], fh);
    }
    return IVX_OK;
}

extern "C" int ivx_slice_dab_clip(int64_t xi, int64_t yi, int64_t fh, int64_t fw, int64_t h, int64_t w, int64_t out[6]) {
    IVX_REQUIRE(fh >= 0 && fw >= 0 && h >= 0 && w >= 0, IVX_EINVAL, "dab_clip: negative size");
    const se::Clip cx = se::clip_axis(xi, fw, w), cy = se::clip_axis(yi, fh, h);
    out[0] = cx.at, out[1] = cx.skip, out[2] = cx.count, out[3] = cy.at, out[4] = cy.skip, out[5] = cy.count;
    return IVX_OK;
}

extern "C" int ivx_slice_dab_extent(int64_t xi, int64_t yi, int64_t fh, int64_t fw, int64_t h, int64_t w, int64_t row_stride,
                                    int64_t elem_stride, int64_t out[3]) {
    IVX_REQUIRE(fh >= 0 && fw >= 0 && h >= 0 && w >= 0, IVX_EINVAL, "dab_extent: negative size");
    int64_t count = 0, lo = -1, hi = -1;
    for (int64_t fy = 0; fy < fh; fy++)
        for (int64_t fx = 0; fx < fw; fx++) {
            int64_t y, x;
            if (!se::dab_pixel(xi, yi, fy, fx, h, w, &y, &x)) continue;
            const int64_t off = se::view_offset(y, x, row_stride, elem_stride);
            lo = count == 0 || off < lo ? off : lo;
            hi = count == 0 || off > hi ? off : hi;
            count++;
        }
    out[0] = count, out[1] = lo, out[2] = hi;
    return IVX_OK;
}

// ---- host forms ---------------------------------------------------------------------------------------------------------------
extern "C" int ivx_mask_brush_stroke(uint8_t *mask, const int64_t image_shape[3], const int64_t mst[3], const int16_t *image,
                                     const int64_t ist[3], int orientation, int64_t n, const uint8_t *footprint, int64_t fh,
                                     int64_t fw, const int32_t *dabs, const int32_t *run_ops, const int64_t *run_lens,
                                     int64_t nruns, int thresh_min, int thresh_max, int fill_value, int padded, int set_flag,
                                     uint8_t *previous) {
    ivx::HostCallGuard host_guard__;
    using namespace ivx;
    IVX_REQUIRE(fh >= 0 && fw >= 0 && nruns >= 0, IVX_EINVAL, "brush_stroke: negative size");
    // `padded`: a mask matrix (one flag plane in front of every axis); otherwise a matrix of the image's own shape (markers)
    SliceGeom g;
    int rc;
    if ((rc = slice_geom(image_shape, mst, image ? ist : nullptr, orientation, n, &g))) return rc;
    if (!padded) {
        g.moff = n * mst[orientation];
        set_flag = 0;
    }
    const size_t npix = (size_t)g.h * g.w;
    if (npix == 0) return IVX_OK;
    int64_t ndabs = 0;
    bool reads = false;
    for (int64_t r = 0; r < nruns; r++) {
        IVX_REQUIRE(run_lens[r] >= 0, IVX_EINVAL, "brush_stroke: negative run length");
        IVX_REQUIRE(run_ops[r] >= se::OP_DRAW && run_ops[r] <= se::OP_FILL, IVX_EINVAL, "brush_stroke: unknown operation %d", run_ops[r]);
        ndabs += run_lens[r];
        reads |= se::op_reads_image(run_ops[r]);
    }
    IVX_REQUIRE(!reads || image, IVX_EINVAL, "brush_stroke: a threshold operation needs the image");
    uint8_t *view = mask + g.moff;
    const int64_t sh[3] = {1, g.h, g.w}, vst[3] = {g.mrs * g.h, g.mrs, g.mes};
    if (previous) { // p_mask of apply_slice_buffer_to_mask: the host copy is the authoritative one, nothing crosses the link
        for (int64_t y = 0; y < g.h; y++)
            for (int64_t x = 0; x < g.w; x++) previous[y * g.w + x] = view[se::view_offset(y, x, g.mrs, g.mes)];
    }
    void *d_m, *d_i = nullptr, *d_f, *d_d;
    if ((rc = ws_get(WS_OUT, npix + 16, &d_m))) return rc;
    if ((rc = upload_strided(d_m, view, sh, vst, 1, WS_OUT))) return rc; // the slice alone; from the mirror when the matrix is bound
    if (reads) {
        const int64_t ivst[3] = {g.irs * g.h, g.irs, g.ies};
        if ((rc = ws_get(WS_IN, npix * 2, &d_i))) return rc;
        if ((rc = upload_strided(d_i, (const uint8_t *)image + g.ioff, sh, ivst, 2, WS_IN))) return rc;
    }
    if (ndabs && fh * fw) {
        if ((rc = ws_get(WS_AUX0, (size_t)(fh * fw), &d_f))) return rc;
        if ((rc = ws_get(WS_SMALL, (size_t)ndabs * 8, &d_d))) return rc;
        if ((rc = copy_h2d(d_f, footprint, (size_t)(fh * fw)))) return rc;
        if ((rc = copy_h2d(d_d, dabs, (size_t)ndabs * 8))) return rc;
        int64_t at = 0;
        for (int64_t r = 0; r < nruns; r++) { // the runs of one operation, in order on one stream: later ones overwrite earlier ones
            if ((rc = ivx_dev_mask_brush_stroke((uint8_t *)d_m, g.w, 1, (const int16_t *)d_i, g.w * 2, 2, g.h, g.w, (const uint8_t *)d_f,
                                                fh, fw, (const int32_t *)d_d + 2 * at, run_lens[r], run_ops[r], thresh_min, thresh_max,
                                                fill_value, nullptr)))
                return rc;
            at += run_lens[r];
        }
    }
    if (set_flag) IVX_HIP(hipMemsetAsync((uint8_t *)d_m + npix, 2, 1, nullptr)); // matrix[n+1, 0, 0] = 2 (slice_.py:1940)
    IVX_HIP(hipDeviceSynchronize());
    if ((rc = download_strided(view, sh, vst, d_m, 1, WS_OUT))) return rc; // host and mirror
    if (set_flag) return copy_d2h(mask + g.flag_off, (const uint8_t *)d_m + npix, 1);
    return IVX_OK;
}

extern "C" int ivx_mask_crop(uint8_t *mask, const int64_t shape[3], const int64_t mst[3], const int64_t box[6]) {
    ivx::HostCallGuard host_guard__;
    using namespace ivx;
    IVX_REQUIRE(shape[0] >= 0 && shape[1] >= 0 && shape[2] >= 0, IVX_EINVAL, "mask_crop: negative shape");
    const size_t n = (size_t)shape[0] * shape[1] * shape[2];
    if (n == 0) return IVX_OK;
    void *d_m;
    int rc;
    if ((rc = ws_get(WS_OUT, n, &d_m))) return rc;
    if ((rc = upload_strided(d_m, mask, shape, mst, 1, WS_OUT))) return rc;
    if ((rc = ivx_dev_mask_crop((uint8_t *)d_m, shape[0], shape[1], shape[2], box, nullptr))) return rc;
    IVX_HIP(hipDeviceSynchronize());
    return download_strided(mask, shape, mst, d_m, 1, WS_OUT);
}
