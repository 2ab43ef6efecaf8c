// k_volren.hip -- volume rendering of the 3-D view (invesalius/data/volume.py:575-707, Volume.LoadVolume with
// vtkFixedPointVolumeRayCastMapper) and the volume histogram (CalculateHistogram, :723-735).
//
// prepare: uint16(img + shift), then the preset's "Basic Smooth 5x5" passes per XY slice (float64, row-major taps,
//          out-of-volume taps skipped, truncated toward zero: bit for bit with tests/_volren_ref.py).
// cells:   min / max of the prepared field per 8^3 macro cell, one voxel of apron on every side.
// render:  one lane per ray, 8x8 pixel tiles per wave; parallel rays, samples t_in + k dt (from k, never accumulated),
//          trilinear interpolation, classification by linear interpolation of the baked table, optional headlight
//          shading from central differences, front-to-back compositing with early termination at A >= 1 - 2^-12, or the
//          maximum intensity.  Empty-space skipping jumps over macro cells whose table entries [min - 1, max + 1] are all
//          transparent (MIP: whose max cannot raise the running maximum); a jump lands only where every skipped sample
//          lies in the cell, so skipping changes no bit.  The rays, the trilinear sample, the
//          headlight, the composite loop, the pixel write, the counters and the cells kernel are volren_ray.h's, read
//          here through its DenseField; the maximum-intensity loop is this file's.
// histogram: uint64 counts, privatised in LDS where the bins fit; integer atomics only.
#include "ivx_internal.h"
#include "volren_ray.h"

using namespace ivx;

namespace {

constexpr int HIST_LDS_BINS = 16384;           // 64 KiB of uint32 counters

struct Kern25 {
    double w[25];
};

// volume.py:52-81 "Basic Smooth 5x5"
const double BASIC_SMOOTH_5X5[25] = {1, 1, 1, 1, 1, 1, 4, 4, 4, 1, 1, 4, 12, 4, 1, 1, 4, 4, 4, 1, 1, 1, 1, 1, 1};

__global__ __launch_bounds__(256) void k_vr_shift(const int16_t *__restrict__ img, int64_t n, int shift,
                                                 uint16_t *__restrict__ out) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = (uint16_t)((int)img[i] + shift);
}

// vtkImageConvolve's 5x5 kernel on every XY slice; block (64, 4) of one slice
__global__ __launch_bounds__(256) void k_vr_smooth(const uint16_t *__restrict__ in, uint16_t *__restrict__ out, Dims d,
                                                  Kern25 k) {
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y, z = blockIdx.z;
    if (x >= d.nx || y >= d.ny) return;
    const uint16_t *sl = in + (int64_t)z * d.ny * d.nx;
    double acc = 0.0;
    for (int ky = 0; ky < 5; ky++) {
        const int yy = y + ky - 2;
        if (yy < 0 || yy >= d.ny) continue;
        for (int kx = 0; kx < 5; kx++) {
            const int xx = x + kx - 2;
            if (xx < 0 || xx >= d.nx) continue;
            acc = acc + k.w[ky * 5 + kx] * (double)sl[(int64_t)yy * d.nx + xx];
        }
    }
    out[((int64_t)z * d.ny + y) * d.nx + x] = (uint16_t)acc;
}

__global__ __launch_bounds__(64) void k_vr_render(const uint16_t *__restrict__ v, const uint16_t *__restrict__ cells, Dims d,
                                                 Dims c, const float4 *__restrict__ table, const float *__restrict__ alpha,
                                                 const uint32_t *__restrict__ prefix, ivx_volren_params p, void *out,
                                                 unsigned long long *stats) {
    const int px = blockIdx.x * TILE + (threadIdx.x & (TILE - 1));
    const int py = blockIdx.y * TILE + (threadIdx.x / TILE);
    const bool active = px < p.width && py < p.height;
    unsigned long long n_taken = 0, n_skipped = 0, n_early = 0, n_hit = 0;
    float r = (float)p.background[0], g = (float)p.background[1], b = (float)p.background[2], A = 0.0f;
    const DenseField fld{v, (int64_t)d.ny * d.nx, d.nx};
    RayCtx ray;
    if (active && setup_ray(p, d, px, py, ray)) {
        n_hit = 1;
        const int nt = p.n_table;
        const float vmaxf = (float)(nt - 2);
        if (p.mip) {
            float vmax = -1.0f;
            for (long long k = 0; k <= ray.kmax;) {
                float x, y, z;
                sample_pos(ray, d, k, x, y, z);
                if (p.skip) {
                    const int cx = (int)x / CELL, cy = (int)y / CELL, cz = (int)z / CELL;
                    const int64_t ci = ((int64_t)cz * c.ny + cy) * c.nx + cx;
                    if ((float)cells[2 * ci + 1] <= vmax) {
                        const long long kn = cell_exit(ray, d, k, cx, cy, cz);
                        n_skipped += (unsigned long long)(kn - k);
                        k = kn;
                        continue;
                    }
                }
                const float s = tri(fld, d, x, y, z);
                n_taken++;
                if (s > vmax) vmax = s;
                k++;
            }
            if (vmax >= 0.0f) {
                const float s = fminf(vmax, vmaxf + 1.0f);
                const int i0 = min((int)s, nt - 2);
                const float f = s - (float)i0;
                const float4 e0 = table[i0], e1 = table[i0 + 1];
                const float a = lerpf(alpha[i0], alpha[i0 + 1], f);
                r = a * lerpf(e0.x, e1.x, f) + (1.0f - a) * r;
                g = a * lerpf(e0.y, e1.y, f) + (1.0f - a) * g;
                b = a * lerpf(e0.z, e1.z, f) + (1.0f - a) * b;
                A = a;
            }
        } else {
            composite_ray(fld, cells, d, c, table, prefix, p, ray, r, g, b, A, n_taken, n_skipped, n_early);
        }
    }
    if (active) write_pixel(out, p, px, py, r, g, b, A);
    add_stats(stats, n_taken, n_skipped, n_early, n_hit);
}

__global__ __launch_bounds__(256) void k_vr_hist_lds(const int16_t *__restrict__ img, int64_t n, int lo, int nbins,
                                                    unsigned long long *__restrict__ counts) {
    __shared__ uint32_t bins[HIST_LDS_BINS];
    for (int i = threadIdx.x; i < nbins; i += blockDim.x) bins[i] = 0;
    __syncthreads();
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int b = (int)img[i] - lo;
        if (b >= 0 && b < nbins) atomicAdd(&bins[b], 1u);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < nbins; i += blockDim.x)
        if (bins[i]) atomicAdd(counts + i, (unsigned long long)bins[i]);
}

__global__ __launch_bounds__(256) void k_vr_hist_global(const int16_t *__restrict__ img, int64_t n, int lo, int nbins,
                                                       unsigned long long *__restrict__ counts) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int b = (int)img[i] - lo;
        if (b >= 0 && b < nbins) atomicAdd(counts + b, 1ull);
    }
}

} // namespace

extern "C" int ivx_dev_volren_prepare(const int16_t *img, const int64_t shape[3], int shift, int nsmooth, uint16_t *out,
                                      uint16_t *scratch, void *stream) {
    Dims d;
    int rc;
    if ((rc = check_shape(shape, d))) return rc;
    IVX_REQUIRE(img && out && (void *)img != (void *)out, IVX_EINVAL, "volren: prepare needs distinct in / out buffers");
    IVX_REQUIRE(nsmooth >= 0 && nsmooth <= 64, IVX_EINVAL, "volren: %d smoothing passes", nsmooth);
    IVX_REQUIRE(nsmooth < 1 || (scratch && (void *)scratch != (void *)out), IVX_EINVAL, "volren: prepare needs scratch");
    IVX_REQUIRE(shift >= 0 && shift <= 65535, IVX_EINVAL, "volren: shift %d", shift);
    const int64_t n = (int64_t)d.nz * d.ny * d.nx;
    hipStream_t st = S(stream);
    // shift, then the passes ping-pong between out and scratch so that the last write lands in out
    uint16_t *bufs[2] = {out, scratch};
    int cur = nsmooth & 1;
    hipLaunchKernelGGL(k_vr_shift, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, st, img, n, shift, bufs[cur]);
    IVX_LAUNCH_CHECK();
    Kern25 k;
    for (int i = 0; i < 25; i++) k.w[i] = BASIC_SMOOTH_5X5[i] / 60.0;
    dim3 grid((unsigned)cdiv(d.nx, 64), (unsigned)cdiv(d.ny, 4), (unsigned)d.nz);
    for (int pass = 0; pass < nsmooth; pass++) {
        const uint16_t *src = bufs[cur];
        cur ^= 1;
        hipLaunchKernelGGL(k_vr_smooth, grid, dim3(64, 4), 0, st, src, bufs[cur], d, k);
        IVX_LAUNCH_CHECK();
    }
    return IVX_OK;
}

extern "C" int ivx_dev_volren_cells(const uint16_t *vol, const int64_t shape[3], uint16_t *cells, void *stream) {
    Dims d;
    int rc;
    if ((rc = check_shape(shape, d))) return rc;
    IVX_REQUIRE(vol && cells, IVX_EINVAL, "volren: null buffer");
    const Dims c = cell_dims(d);
    const int64_t nc = (int64_t)c.nz * c.ny * c.nx;
    const DenseField f{vol, (int64_t)d.ny * d.nx, d.nx};
    hipLaunchKernelGGL(k_cells<DenseField>, dim3((unsigned)cdiv(nc, 256)), dim3(256), 0, S(stream), f, d, c, 0, nc, cells);
    IVX_LAUNCH_CHECK();
    return IVX_OK;
}

extern "C" int ivx_dev_volren_render(const uint16_t *vol, const uint16_t *cells, const int64_t shape[3], const float *table,
                                     const float *alpha, const uint32_t *prefix, const ivx_volren_params *p, void *out,
                                     uint64_t *stats, void *stream) {
    Dims d;
    int rc;
    if ((rc = check_shape(shape, d)) || (rc = check_params(p))) return rc;
    IVX_REQUIRE(vol && table && alpha && out, IVX_EINVAL, "volren: null buffer");
    IVX_REQUIRE(!p->skip || (cells && prefix), IVX_EINVAL, "volren: skipping needs the cells and the prefix counts");
    const Dims c = cell_dims(d);
    dim3 grid((unsigned)cdiv(p->width, TILE), (unsigned)cdiv(p->height, TILE));
    hipLaunchKernelGGL(k_vr_render, grid, dim3(TILE * TILE), 0, S(stream), vol, cells, d, c, (const float4 *)table, alpha,
                       prefix, *p, out, (unsigned long long *)stats);
    IVX_LAUNCH_CHECK();
    return IVX_OK;
}

extern "C" int ivx_dev_volren_histogram(const int16_t *img, int64_t n, int lo, int nbins, uint64_t *counts, void *stream) {
    IVX_REQUIRE(n >= 0 && nbins >= 0 && nbins <= 65536, IVX_EINVAL, "volren: histogram of %lld voxels, %d bins", (long long)n,
                nbins);
    if (nbins == 0) return IVX_OK;
    IVX_REQUIRE(img && counts, IVX_EINVAL, "volren: null buffer");
    hipStream_t st = S(stream);
    IVX_HIP(hipMemsetAsync(counts, 0, (size_t)nbins * 8, st));
    if (n == 0) return IVX_OK;
    const int64_t nb = cdiv(n, 256 * 16);
    const unsigned blocks = (unsigned)(nb < 2048 ? nb : 2048);
    if (nbins <= HIST_LDS_BINS)
        hipLaunchKernelGGL(k_vr_hist_lds, dim3(blocks), dim3(256), 0, st, img, n, lo, nbins, (unsigned long long *)counts);
    else
        hipLaunchKernelGGL(k_vr_hist_global, dim3(blocks), dim3(256), 0, st, img, n, lo, nbins, (unsigned long long *)counts);
    IVX_LAUNCH_CHECK();
    return IVX_OK;
}

extern "C" int ivx_volume_render(const int16_t *img, const int64_t shape[3], const int64_t strides[3], int shift, int nsmooth,
                                 const float *table, const float *alpha, const uint32_t *prefix, const ivx_volren_params *p,
                                 void *out) {
    HostCallGuard guard;
    Dims d;
    int rc;
    if ((rc = check_shape(shape, d)) || (rc = check_params(p))) return rc;
    IVX_REQUIRE(img && strides && table && alpha && prefix && out, IVX_EINVAL, "volren: null buffer");
    const int64_t n = (int64_t)d.nz * d.ny * d.nx;
    const Dims c = cell_dims(d);
    const size_t ncell = (size_t)c.nz * c.ny * c.nx;
    const size_t nt = (size_t)p->n_table;
    const size_t tb = nt * 16, ab = nt * 4, pb = (nt + 1) * 4;
    const size_t ob = (size_t)p->width * p->height * 4 * (p->out_u8 ? 1 : 4);
    void *d_in, *d_vol, *d_s, *d_cells, *d_lut, *d_out;
    if ((rc = ws_get(WS_IN, (size_t)n * 2, &d_in)) || (rc = ws_get(WS_AUX0, (size_t)n * 2, &d_vol)) ||
        (rc = ws_get(WS_AUX1, (size_t)n * 2, &d_s)) || (rc = ws_get(WS_AUX2, ncell * 4, &d_cells)) ||
        (rc = ws_get(WS_LUT, tb + ab + pb, &d_lut)) || (rc = ws_get(WS_OUT, ob, &d_out)))
        return rc;
    if ((rc = upload_strided(d_in, img, shape, strides, 2, WS_IN))) return rc;
    char *lut = (char *)d_lut;
    if ((rc = copy_h2d(lut, table, tb)) || (rc = copy_h2d(lut + tb, alpha, ab)) || (rc = copy_h2d(lut + tb + ab, prefix, pb)))
        return rc;
    if ((rc = ivx_dev_volren_prepare((const int16_t *)d_in, shape, shift, nsmooth, (uint16_t *)d_vol, (uint16_t *)d_s, nullptr)))
        return rc;
    if ((rc = ivx_dev_volren_cells((const uint16_t *)d_vol, shape, (uint16_t *)d_cells, nullptr))) return rc;
    if ((rc = ivx_dev_volren_render((const uint16_t *)d_vol, (const uint16_t *)d_cells, shape, (const float *)lut,
                                    (const float *)(lut + tb), (const uint32_t *)(lut + tb + ab), p, d_out, nullptr, nullptr)))
        return rc;
    IVX_HIP(hipDeviceSynchronize());
    return copy_d2h(out, d_out, ob);
}
