// k_maskren.hip -- the mask 3-D preview (invesalius/data/volume_mask.py:36-119, VolumeMask.create_volume): ray casting of
// the uint8 mask, read in place.
//
// field:  a uint8 base pointer with byte strides (the padded host matrix and the dense device mask go in without a copy)
//         and an optional virtual leading apron: one plane at index 0 of every axis that holds a constant byte, so that
//         positions count as for the padded matrix while DeviceVolume keeps the mask dense.
// cells:  min / max bytes per 8^3 macro cell, one voxel of apron on every side; a z range rebuilds only the cells that a
//         slab edit touched.
// render: one lane per ray, 8x8 pixel tiles per wave; the rays, samples, headlight, pixel write and counters are
//         volren_ray.h's, read through its Field, as is the cells kernel.
//         composite: volren_ray.h's composite_ray, the one loop k_volren.hip runs too (so the same bits on the same
//                    values).  A cell is skipped when the table entries [min, max] are all transparent: a byte field
//                    sampled at an integer s has fraction 0, so entry floor(s) + 1 weighs nothing at s == max.
//         iso:       the first sample k >= 1 with (f[k-1] - 127)(f[k] - 127) < 0 or f[k] == 127; one linear step to the
//                    hit, the gradient and the headlight there, alpha 1, and the hit's distance as depth.  A cell whose
//                    bytes lie all below or all above 127 holds no crossing; it is jumped when the predecessor lies on the
//                    same side, and the predecessor's value is sampled again when a crossing needs it, so skipping
//                    changes no bit.
#include "ivx_internal.h"
#include "volren_ray.h"

using namespace ivx;

namespace {

constexpr float ISO = 127.0f; // SetValue(0, 127), volume_mask.py:103

template <bool ISOMODE>
__global__ __launch_bounds__(64) void k_mr_render(Field v, const uint8_t *__restrict__ cells, Dims d, Dims c,
                                                 const float4 *__restrict__ table, const uint32_t *__restrict__ prefix,
                                                 ivx_volren_params p, void *out, float *__restrict__ depth,
                                                 unsigned long long *stats) {
    const int px = blockIdx.x * TILE + (threadIdx.x & (TILE - 1));
    const int py = blockIdx.y * TILE + (threadIdx.x / TILE);
    const bool active = px < p.width && py < p.height;
    unsigned long long n_taken = 0, n_skipped = 0, n_early = 0, n_hit = 0;
    float r = (float)p.background[0], g = (float)p.background[1], b = (float)p.background[2], A = 0.0f;
    float t_hit = __builtin_inff();
    RayCtx ray;
    if (active && setup_ray(p, d, px, py, ray)) {
        n_hit = 1;
        if (ISOMODE) {
            const Light l = make_light(p, d);
            // side: that of f[k - 1] - 127 (-1 / 0 / +1); f_prev is its value while have_prev
            int side = 0;
            bool have_prev = false;
            float f_prev = 0.0f;
            for (long long k = 0; k <= ray.kmax;) {
                float x, y, z;
                sample_pos(ray, d, k, x, y, z);
                if (p.skip) {
                    const int cx = (int)x / CELL, cy = (int)y / CELL, cz = (int)z / CELL;
                    const int64_t ci = ((int64_t)cz * c.ny + cy) * c.nx + cx;
                    const int cs = (float)cells[2 * ci + 1] < ISO ? -1 : ((float)cells[2 * ci] > ISO ? 1 : 0);
                    if (cs != 0 && (k == 0 || side == cs)) {
                        const long long kn = cell_exit(ray, d, k, cx, cy, cz);
                        n_skipped += (unsigned long long)(kn - k);
                        k = kn;
                        side = cs;
                        have_prev = false;
                        continue;
                    }
                }
                const float f = tri(v, d, x, y, z);
                n_taken++;
                const int s = f < ISO ? -1 : (f > ISO ? 1 : 0);
                if (k >= 1 && (s == 0 || s * side < 0)) {
                    float w = 1.0f, hx = x, hy = y, hz = z;
                    if (s != 0) {
                        float x0, y0, z0;
                        sample_pos(ray, d, k - 1, x0, y0, z0);
                        if (!have_prev) { // jumped over: the same value as without skipping
                            f_prev = tri(v, d, x0, y0, z0);
                            n_taken++;
                        }
                        w = (ISO - f_prev) / (f - f_prev);
                        hx = x0 + w * (x - x0);
                        hy = y0 + w * (y - y0);
                        hz = z0 + w * (z - z0);
                    }
                    const float4 e0 = table[127];
                    r = e0.x, g = e0.y, b = e0.z;
                    if (p.shade) shade_at(v, d, l, hx, hy, hz, r, g, b);
                    A = 1.0f;
                    t_hit = (float)(ray.tin + ((double)(k - 1) + (double)w) * p.dt);
                    n_early = 1;
                    break;
                }
                side = s;
                f_prev = f;
                have_prev = true;
                k++;
            }
        } else {
            composite_ray(v, cells, d, c, table, prefix, p, ray, r, g, b, A, n_taken, n_skipped, n_early);
        }
    }
    if (active) {
        write_pixel(out, p, px, py, r, g, b, A);
        if (ISOMODE && depth) depth[(int64_t)py * p.width + px] = t_hit;
    }
    add_stats(stats, n_taken, n_skipped, n_early, n_hit);
}

// the array's shape and strides with the apron as the logical field
int make_field(const uint8_t *mask, const int64_t shape[3], const int64_t strides[3], int apron, int apron_value, Field &f,
               Dims &d) {
    IVX_REQUIRE(shape && strides && mask, IVX_EINVAL, "maskren: null argument");
    IVX_REQUIRE(apron == 0 || apron == 1, IVX_EINVAL, "maskren: apron %d (0 or 1)", apron);
    IVX_REQUIRE(apron_value >= 0 && apron_value <= 255, IVX_EINVAL, "maskren: apron value %d", apron_value);
    const int64_t logical[3] = {shape[0] + apron, shape[1] + apron, shape[2] + apron};
    for (int a = 0; a < 3; a++) IVX_REQUIRE(shape[a] >= 1, IVX_EINVAL, "maskren: shape[%d] = %lld", a, (long long)shape[a]);
    int rc;
    if ((rc = check_shape(logical, d))) return rc;
    f.base = mask;
    f.sz = strides[0], f.sy = strides[1], f.sx = strides[2];
    f.apron = apron;
    f.av = (unsigned)apron_value;
    return IVX_OK;
}

} // namespace

extern "C" int ivx_dev_maskren_cells(const uint8_t *mask, const int64_t shape[3], const int64_t strides[3], int apron,
                                     int apron_value, int64_t z0, int64_t z1, uint8_t *cells, void *stream) {
    Field f;
    Dims d;
    int rc;
    if ((rc = make_field(mask, shape, strides, apron, apron_value, f, d))) return rc;
    IVX_REQUIRE(cells, IVX_EINVAL, "maskren: null buffer");
    const Dims c = cell_dims(d);
    int cz0 = 0, cz1 = c.nz - 1;
    if (z1 >= 0) { // logical slices [z0, z1): the cells whose voxels with apron, cz CELL - 1 .. cz CELL + CELL, meet them
        IVX_REQUIRE(z0 >= 0 && z0 <= z1 && z1 <= d.nz, IVX_EINVAL, "maskren: z range [%lld, %lld) of %d slices", (long long)z0,
                    (long long)z1, d.nz);
        if (z0 == z1) return IVX_OK;
        cz0 = (int)(z0 >= 1 ? (z0 - 1) / CELL : 0);
        cz1 = (int)((z1 / CELL) < c.nz - 1 ? (z1 / CELL) : c.nz - 1);
    }
    const int64_t nc = (int64_t)(cz1 - cz0 + 1) * c.ny * c.nx;
    hipLaunchKernelGGL(k_cells<Field>, dim3((unsigned)cdiv(nc, 256)), dim3(256), 0, S(stream), f, d, c, cz0, nc, cells);
    IVX_LAUNCH_CHECK();
    return IVX_OK;
}

extern "C" int ivx_dev_maskren_render(const uint8_t *mask, const uint8_t *cells, const int64_t shape[3],
                                      const int64_t strides[3], int apron, int apron_value, int iso, const float *table,
                                      const uint32_t *prefix, const ivx_volren_params *p, void *out, float *depth,
                                      uint64_t *stats, void *stream) {
    Field f;
    Dims d;
    int rc;
    if ((rc = make_field(mask, shape, strides, apron, apron_value, f, d)) || (rc = check_params(p))) return rc;
    IVX_REQUIRE(table && out, IVX_EINVAL, "maskren: null buffer");
    IVX_REQUIRE(p->n_table >= 257, IVX_EINVAL, "maskren: n_table %d (a byte reads entries 0 .. 256)", p->n_table);
    IVX_REQUIRE(!p->mip && !p->clip, IVX_EINVAL, "maskren: no maximum intensity mode and no clip plane");
    IVX_REQUIRE(!p->skip || (cells && (iso || prefix)), IVX_EINVAL, "maskren: skipping needs the cells and the prefix counts");
    IVX_REQUIRE(iso || !depth, IVX_EINVAL, "maskren: depth is an output of the iso mode");
    const Dims c = cell_dims(d);
    dim3 grid((unsigned)cdiv(p->width, TILE), (unsigned)cdiv(p->height, TILE));
    if (iso)
        hipLaunchKernelGGL(k_mr_render<true>, grid, dim3(TILE * TILE), 0, S(stream), f, cells, d, c, (const float4 *)table,
                           prefix, *p, out, depth, (unsigned long long *)stats);
    else
        hipLaunchKernelGGL(k_mr_render<false>, grid, dim3(TILE * TILE), 0, S(stream), f, cells, d, c, (const float4 *)table,
                           prefix, *p, out, depth, (unsigned long long *)stats);
    IVX_LAUNCH_CHECK();
    return IVX_OK;
}

extern "C" int ivx_mask_preview(const uint8_t *matrix, const int64_t shape[3], const int64_t strides[3], int iso,
                                const float *table, const uint32_t *prefix, const ivx_volren_params *p, void *out,
                                float *depth) {
    HostCallGuard guard;
    Dims d;
    int rc;
    if ((rc = check_shape(shape, d)) || (rc = check_params(p))) return rc;
    IVX_REQUIRE(matrix && strides && table && prefix && out, IVX_EINVAL, "maskren: null buffer");
    const int64_t n = (int64_t)d.nz * d.ny * d.nx;
    const Dims c = cell_dims(d);
    const size_t ncell = (size_t)c.nz * c.ny * c.nx;
    const size_t nt = (size_t)p->n_table;
    const size_t tb = nt * 16, pb = (nt + 1) * 4;
    const size_t npix = (size_t)p->width * p->height;
    const size_t ob = npix * 4 * (p->out_u8 ? 1 : 4);
    void *d_in, *d_cells, *d_lut, *d_out, *d_depth = nullptr;
    if ((rc = ws_get(WS_IN, (size_t)n, &d_in)) || (rc = ws_get(WS_AUX2, ncell * 2, &d_cells)) ||
        (rc = ws_get(WS_LUT, tb + pb, &d_lut)) || (rc = ws_get(WS_OUT, ob, &d_out)))
        return rc;
    if (depth && (rc = ws_get(WS_AUX0, npix * 4, &d_depth))) return rc;
    if ((rc = upload_strided(d_in, matrix, shape, strides, 1, WS_IN))) return rc;
    char *lut = (char *)d_lut;
    if ((rc = copy_h2d(lut, table, tb)) || (rc = copy_h2d(lut + tb, prefix, pb))) return rc;
    const int64_t dense[3] = {(int64_t)d.ny * d.nx, d.nx, 1};
    if ((rc = ivx_dev_maskren_cells((const uint8_t *)d_in, shape, dense, 0, 0, 0, -1, (uint8_t *)d_cells, nullptr))) return rc;
    if ((rc = ivx_dev_maskren_render((const uint8_t *)d_in, (const uint8_t *)d_cells, shape, dense, 0, 0, iso,
                                     (const float *)lut, (const uint32_t *)(lut + tb), p, d_out, (float *)d_depth, nullptr,
                                     nullptr)))
        return rc;
    IVX_HIP(hipDeviceSynchronize());
    if ((rc = copy_d2h(out, d_out, ob))) return rc;
    return depth ? copy_d2h(depth, d_depth, npix * 4) : IVX_OK;
}
