// k_imagegeo.hip -- the image geometry tools: flip, swap axes and the gantry-tilt correction, the three
// operations of the reference that rewrite the whole image.
//
// Reference semantics (byte-exact):
//   flip         Slice.OnFlipVolume (invesalius/data/slice_.py:2103-2149): m[:] = m[::-1] / m[:, ::-1] / m[:, :, ::-1]
//   swap axes    Slice.OnSwapVolumeAxes (:2151-2251): np.array(m.swapaxes(a, b))
//   gantry tilt  imagedata_utils.FixGantryTilt (imagedata_utils.py:143-154): one scipy.ndimage.shift per slice, cubic spline,
//                cval = the matrix's minimum as it stands before that slice
//
// MI355X design.  Flip and swap are streams: every element is read once and written once, so the only questions are whether
// both sides are coalesced and how wide a lane's access is.
//   flip 0 / 1   whole lines (planes, rows) change places pairwise, in place: lane = one unit of a line, the widest of
//                16 / 8 / 4 / 2 / 1 bytes that divides the line and the block's address.  An odd count leaves the middle line.
//   flip 2       reverses inside a row: lane = one pair of 16-byte chunks (c, last - c), each reversed in registers and
//                stored in the other's place; both are whole aligned chunks when the row is a multiple of 16 bytes.  Every
//                other width takes one pair of elements per lane: odd widths, unaligned rows, widths below a chunk.
//   swap (1, 0)  moves whole x-rows: the same unit copy, loads and stores both coalesced, no staging.
//   swap (2, 1), (2, 0)  transposes with the contiguous axis: a 64 x 64 tile goes through LDS, rows in (64 lanes along the
//                source's x), columns out (64 lanes along the destination's contiguous axis).  The tile's pitch is 64
//                elements plus 4 bytes, an odd number of dwords for 1-, 2- and 4-byte elements: the column read of 32 lanes
//                then falls on 32 different banks ((a / 4) % 32 for the narrow LDS reads), where a pitch of 65 int16 -- 32.5
//                dwords -- would put lanes 2k and 2k + 1 on one bank.
//   tilt         the y recursion is serial per column and parallel over x and z: lane = one column of one slice, the 64
//                lanes of a wave along x, so every step's load and store is one coalesced line.  The column's float64
//                coefficients live in a scratch slab [slice][y][x]; the column is read (causal initialisation over the whole
//                line, then the causal pass), its coefficients are written, rewritten by the anti-causal pass and gathered by
//                the four taps, and the int16 result replaces the column in place.  The same pass leaves each slice's
//                original minimum and the minimum of the rows it wrote (wave minimum, one atomicMin per wave: a minimum does
//                not depend on the order).  The chain of fill values is D numbers: they go to the host, which resolves it
//                (imagegeo_math.h), and a fill pass writes the rows that fall outside.  pole ** (H - 1) comes from the host's
//                C library, as the reference forms it.  A lane's arithmetic does not depend on the launch shape.
#include <algorithm>
#include <vector>

#include "imagegeo_math.h"
#include "ivx_internal.h"

namespace ig = ivx_imagegeo;

namespace {

// ---- flip -----------------------------------------------------------------------------------------------------------------------
// v as [O][N][L units]: line p of every outer block changes places with line N - 1 - p
template <typename U> __global__ __launch_bounds__(256) void k_flip_lines(U *v, int64_t O, int64_t N, int64_t L) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x, P = N / 2;
    if (i >= O * P * L) return;
    const int64_t u = i % L, r = i / L, p = r % P, o = r / P;
    U *a = v + (o * N + p) * L + u, *b = v + (o * N + (N - 1 - p)) * L + u;
    const U t = *a;
    *a = *b;
    *b = t;
}

// rows of W elements: element x changes places with W - 1 - x
template <typename T> __global__ __launch_bounds__(256) void k_flip_row_elems(T *v, int64_t R, int64_t W) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x, P = W / 2;
    if (i >= R * P) return;
    const int64_t x = i % P, r = i / P;
    T *a = v + r * W + x, *b = v + r * W + (W - 1 - x);
    const T t = *a;
    *a = *b;
    *b = t;
}

template <typename T> struct Chunk {
    static constexpr int E = 16 / (int)sizeof(T);
    union {
        uint4 q;
        T e[E];
    };
    __device__ void reverse() {
#pragma unroll
        for (int k = 0; k < E / 2; k++) {
            const T t = e[k];
            e[k] = e[E - 1 - k];
            e[E - 1 - k] = t;
        }
    }
};
// rows of C aligned 16-byte chunks: chunk c, reversed, changes places with chunk C - 1 - c, reversed
template <typename T> __global__ __launch_bounds__(256) void k_flip_row_chunks(uint4 *v, int64_t R, int64_t C) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x, P = (C + 1) / 2;
    if (i >= R * P) return;
    const int64_t c = i % P, r = i / P;
    uint4 *a = v + r * C + c, *b = v + r * C + (C - 1 - c);
    Chunk<T> x, y;
    x.q = *a;
    x.reverse();
    if (a == b) { // the middle chunk of an odd count
        *a = x.q;
        return;
    }
    y.q = *b;
    y.reverse();
    *a = y.q;
    *b = x.q;
}

// ---- swap -----------------------------------------------------------------------------------------------------------------------
// (1, 0): out[y][z][:] = in[z][y][:], rows of L units
template <typename U> __global__ __launch_bounds__(256) void k_swap_rows(const U *__restrict__ in, U *__restrict__ out, int64_t D, int64_t H, int64_t L) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= D * H * L) return;
    const int64_t u = i % L, r = i / L, y = r % H, z = r / H;
    out[(y * D + z) * L + u] = in[i];
}

constexpr int TILE = 64;
template <typename T> constexpr int tile_pitch() { return TILE + (sizeof(T) < 4 ? 4 / (int)sizeof(T) : 1); }
// out[b * obs + c * ocs + r] = in[b * ibs + r * irs + c] for b < B, r < R, c < C (strides in elements)
template <typename T>
__global__ __launch_bounds__(256) void k_transpose(const T *__restrict__ in, T *__restrict__ out, int64_t B, int64_t R, int64_t C, int64_t ibs,
                                                   int64_t irs, int64_t obs, int64_t ocs) {
    __shared__ T tile[TILE][tile_pitch<T>()];
    const int64_t tc = (C + TILE - 1) / TILE, tr = (R + TILE - 1) / TILE;
    const int64_t blk = blockIdx.x, b = blk / (tr * tc), t = blk % (tr * tc);
    const int64_t r0 = (t / tc) * TILE, c0 = (t % tc) * TILE;
    const int tx = threadIdx.x % TILE, ty = threadIdx.x / TILE; // 64 x 4
    if (b >= B) return;
    for (int k = ty; k < TILE; k += 4) {
        const int64_t r = r0 + k, c = c0 + tx;
        if (r < R && c < C) tile[k][tx] = in[b * ibs + r * irs + c];
    }
    __syncthreads();
    for (int k = ty; k < TILE; k += 4) {
        const int64_t c = c0 + k, r = r0 + tx;
        if (c < C && r < R) out[b * obs + c * ocs + r] = tile[tx][k];
    }
}

// ---- gantry tilt ----------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int wave_min(int v) {
    for (int o = 32; o > 0; o >>= 1) {
        const int w = __shfl_xor(v, o, 64);
        v = w < v ? w : v;
    }
    return v;
}

// slices z0 .. z0 + nz - 1: every column's interior rows in place, and the two minima of every slice
__global__ __launch_bounds__(64) void k_tilt_columns(int16_t *img, int64_t z0, int64_t nz, int64_t H, int64_t W, const double *__restrict__ nshift,
                                                     double zn1, double *scratch, int *old_min, int *new_min) {
    const int64_t xb = (W + 63) / 64;
    const int64_t zl = (int64_t)blockIdx.x / xb, x = ((int64_t)blockIdx.x % xb) * 64 + threadIdx.x;
    if (zl >= nz) return; // (whole workgroups: the wave minimum below sees all its lanes)
    const int64_t z = z0 + zl;
    int imin = ig::NO_MIN, omin = ig::NO_MIN;
    if (x < W) ig::shift_column(img + z * H * W + x, W, scratch + zl * H * W + x, W, H, nshift[z], zn1, &imin, &omin);
    imin = wave_min(imin);
    omin = wave_min(omin);
    if (threadIdx.x == 0) {
        atomicMin(&old_min[z], imin);
        atomicMin(&new_min[z], omin);
    }
}

// the rows whose source coordinate falls outside the slice: cval[z]
__global__ __launch_bounds__(256) void k_tilt_fill(int16_t *img, int64_t D, int64_t H, int64_t W, const double *__restrict__ nshift,
                                                   const int *__restrict__ cval) {
    const int64_t row = blockIdx.x; // z * H + y
    if (row >= D * H) return;
    const int64_t z = row / H, y = row % H;
    double cc;
    if (ig::row_source(y, nshift[z], H, &cc)) return;
    const int16_t v = (int16_t)cval[z];
    for (int64_t x = threadIdx.x; x < W; x += 256) img[row * W + x] = v;
}

template <typename K, typename... A> int launch1d(K kernel, int64_t threads, int block, hipStream_t st, const char *what, A... args) {
    const int64_t blocks = ivx::cdiv(threads, block);
    IVX_REQUIRE(blocks < ((int64_t)1 << 31), IVX_EINVAL, "%s: %lld workgroups", what, (long long)blocks);
    if (blocks <= 0) return IVX_OK;
    hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3((unsigned)block), 0, st, args...);
    IVX_LAUNCH_CHECK();
    return IVX_OK;
}

// the widest unit that divides a line of `bytes` bytes and the addresses
int unit_of(int64_t bytes, uintptr_t a, uintptr_t b) {
    for (int u = 16; u > 1; u >>= 1)
        if (bytes % u == 0 && a % u == 0 && b % u == 0) return u;
    return 1;
}

bool check_dims(const char *what, int64_t dz, int64_t dy, int64_t dx, size_t isz) {
    if (dz < 0 || dy < 0 || dx < 0) {
        ivx::set_error("%s: negative shape", what);
        return false;
    }
    if (isz != 1 && isz != 2 && isz != 4 && isz != 8) {
        ivx::set_error("%s: item size %zu (1, 2, 4 or 8)", what, isz);
        return false;
    }
    if (dz && dy && dx && (double)dz * (double)dy * (double)dx * (double)isz >= 4.0e18) {
        ivx::set_error("%s: volume too large", what);
        return false;
    }
    return true;
}

int flip_lines(void *v, int64_t O, int64_t N, int64_t bytes, hipStream_t st) {
    if (N < 2 || O == 0 || bytes == 0) return IVX_OK;
    const int u = unit_of(bytes, (uintptr_t)v, 0);
    const int64_t L = bytes / u, threads = O * (N / 2) * L;
    switch (u) {
    case 16: return launch1d(k_flip_lines<uint4>, threads, 256, st, "image_flip", (uint4 *)v, O, N, L);
    case 8: return launch1d(k_flip_lines<uint64_t>, threads, 256, st, "image_flip", (uint64_t *)v, O, N, L);
    case 4: return launch1d(k_flip_lines<uint32_t>, threads, 256, st, "image_flip", (uint32_t *)v, O, N, L);
    case 2: return launch1d(k_flip_lines<uint16_t>, threads, 256, st, "image_flip", (uint16_t *)v, O, N, L);
    }
    return launch1d(k_flip_lines<uint8_t>, threads, 256, st, "image_flip", (uint8_t *)v, O, N, L);
}

template <typename T> int flip_rows(void *v, int64_t R, int64_t W, hipStream_t st) {
    if (W < 2 || R == 0) return IVX_OK;
    if ((W * (int64_t)sizeof(T)) % 16 == 0 && (uintptr_t)v % 16 == 0) {
        const int64_t C = W * (int64_t)sizeof(T) / 16;
        return launch1d(k_flip_row_chunks<T>, R * ((C + 1) / 2), 256, st, "image_flip", (uint4 *)v, R, C);
    }
    return launch1d(k_flip_row_elems<T>, R * (W / 2), 256, st, "image_flip", (T *)v, R, W);
}

template <typename T>
int transpose(const void *in, void *out, int64_t B, int64_t R, int64_t C, int64_t ibs, int64_t irs, int64_t obs, int64_t ocs, hipStream_t st) {
    const int64_t blocks = B * ivx::cdiv(R, TILE) * ivx::cdiv(C, TILE);
    return launch1d(k_transpose<T>, blocks * 256, 256, st, "image_swap_axes", (const T *)in, (T *)out, B, R, C, ibs, irs, obs, ocs);
}

size_t tilt_header_bytes(int64_t dz) { return (((size_t)dz * (3 * sizeof(int) + sizeof(double))) + 255) & ~(size_t)255; }
constexpr size_t TILT_SLAB_BYTES = (size_t)512 << 20; // the coefficient slab a launch works in, at most

} // namespace

extern "C" int ivx_dev_image_flip(void *vol, int64_t dz, int64_t dy, int64_t dx, size_t isz, int axis, void *stream) {
    IVX_REQUIRE(axis >= 0 && axis <= 2, IVX_EINVAL, "image_flip: axis %d (0, 1 or 2)", axis);
    if (!check_dims("image_flip", dz, dy, dx, isz)) return IVX_EINVAL;
    if (dz * dy * dx == 0) return IVX_OK;
    IVX_REQUIRE(vol && (uintptr_t)vol % isz == 0, IVX_EINVAL, "image_flip: null or misaligned block");
    hipStream_t st = ivx::S(stream);
    if (axis == 0) return flip_lines(vol, 1, dz, dy * dx * (int64_t)isz, st);
    if (axis == 1) return flip_lines(vol, dz, dy, dx * (int64_t)isz, st);
    switch (isz) {
    case 1: return flip_rows<uint8_t>(vol, dz * dy, dx, st);
    case 2: return flip_rows<uint16_t>(vol, dz * dy, dx, st);
    case 4: return flip_rows<uint32_t>(vol, dz * dy, dx, st);
    }
    return flip_rows<uint64_t>(vol, dz * dy, dx, st);
}

extern "C" int ivx_dev_image_swap_axes(const void *src, int64_t dz, int64_t dy, int64_t dx, size_t isz, int a, int b, void *dst,
                                       void *stream) {
    IVX_REQUIRE(a >= 0 && a <= 2 && b >= 0 && b <= 2 && a != b, IVX_EINVAL, "image_swap_axes: axes (%d, %d)", a, b);
    if (!check_dims("image_swap_axes", dz, dy, dx, isz)) return IVX_EINVAL;
    if (dz * dy * dx == 0) return IVX_OK;
    IVX_REQUIRE(src && dst && (uintptr_t)src % isz == 0 && (uintptr_t)dst % isz == 0, IVX_EINVAL, "image_swap_axes: null or misaligned block");
    const uintptr_t s0 = (uintptr_t)src, d0 = (uintptr_t)dst, nb = (uintptr_t)(dz * dy * dx) * isz;
    IVX_REQUIRE(s0 + nb <= d0 || d0 + nb <= s0, IVX_EINVAL, "image_swap_axes: source and destination overlap");
    hipStream_t st = ivx::S(stream);
    const int lo = a < b ? a : b, hi = a < b ? b : a;
    if (lo == 0 && hi == 1) { // whole rows
        const int u = unit_of(dx * (int64_t)isz, s0, d0);
        const int64_t L = dx * (int64_t)isz / u, threads = dz * dy * L;
        switch (u) {
        case 16: return launch1d(k_swap_rows<uint4>, threads, 256, st, "image_swap_axes", (const uint4 *)src, (uint4 *)dst, dz, dy, L);
        case 8: return launch1d(k_swap_rows<uint64_t>, threads, 256, st, "image_swap_axes", (const uint64_t *)src, (uint64_t *)dst, dz, dy, L);
        case 4: return launch1d(k_swap_rows<uint32_t>, threads, 256, st, "image_swap_axes", (const uint32_t *)src, (uint32_t *)dst, dz, dy, L);
        case 2: return launch1d(k_swap_rows<uint16_t>, threads, 256, st, "image_swap_axes", (const uint16_t *)src, (uint16_t *)dst, dz, dy, L);
        }
        return launch1d(k_swap_rows<uint8_t>, threads, 256, st, "image_swap_axes", (const uint8_t *)src, (uint8_t *)dst, dz, dy, L);
    }
    // out[z][x][y] = in[z][y][x]: batches z, rows y;  out[x][y][z] = in[z][y][x]: batches y, rows z
    const int64_t B = lo == 1 ? dz : dy, R = lo == 1 ? dy : dz, C = dx;
    const int64_t ibs = lo == 1 ? dy * dx : dx, irs = lo == 1 ? dx : dy * dx;
    const int64_t obs = lo == 1 ? dx * dy : dz, ocs = lo == 1 ? dy : dy * dz;
    switch (isz) {
    case 1: return transpose<uint8_t>(src, dst, B, R, C, ibs, irs, obs, ocs, st);
    case 2: return transpose<uint16_t>(src, dst, B, R, C, ibs, irs, obs, ocs, st);
    case 4: return transpose<uint32_t>(src, dst, B, R, C, ibs, irs, obs, ocs, st);
    }
    return transpose<uint64_t>(src, dst, B, R, C, ibs, irs, obs, ocs, st);
}

extern "C" int ivx_image_tilt_scratch_bytes(int64_t dz, int64_t dy, int64_t dx, size_t *nbytes) {
    IVX_REQUIRE(nbytes, IVX_EINVAL, "image_tilt_scratch_bytes: null");
    if (!check_dims("image_tilt_scratch_bytes", dz, dy, dx, 8)) return IVX_EINVAL;
    const size_t slice = (size_t)dy * dx * sizeof(double);
    int64_t per = slice ? (int64_t)(TILT_SLAB_BYTES / slice) : dz;
    per = std::max<int64_t>(1, std::min(per, dz));
    *nbytes = tilt_header_bytes(dz) + (size_t)per * slice;
    return IVX_OK;
}

extern "C" int ivx_dev_image_fix_gantry_tilt(int16_t *vol, int64_t dz, int64_t dy, int64_t dx, const double *shifts, void *scratch,
                                             size_t scratch_bytes, int *cvals_out, void *stream) {
    if (!check_dims("image_fix_gantry_tilt", dz, dy, dx, 8)) return IVX_EINVAL;
    if (dz * dy * dx == 0) return IVX_OK;
    IVX_REQUIRE(vol && shifts && scratch, IVX_EINVAL, "image_fix_gantry_tilt: null");
    IVX_REQUIRE((uintptr_t)vol % 2 == 0 && (uintptr_t)scratch % 8 == 0, IVX_EINVAL, "image_fix_gantry_tilt: misaligned block");
    const size_t head = tilt_header_bytes(dz), slice = (size_t)dy * dx * sizeof(double);
    IVX_REQUIRE(scratch_bytes >= head + slice, IVX_EINVAL, "image_fix_gantry_tilt: %zu bytes of scratch, at least %zu", scratch_bytes, head + slice);
    const int64_t per = std::min<int64_t>(dz, (int64_t)((scratch_bytes - head) / slice));
    hipStream_t st = ivx::S(stream);
    // the head of the scratch: the negated shifts, then the slices' original minima, written minima and fill values
    double *d_nshift = (double *)scratch;
    int *d_old = (int *)(d_nshift + dz), *d_new = d_old + dz, *d_cval = d_new + dz;
    double *d_coef = (double *)((char *)scratch + head);
    std::vector<double> nshift((size_t)dz);
    for (int64_t n = 0; n < dz; n++) nshift[(size_t)n] = -shifts[n]; // (the reference negates before it calls its C code)
    IVX_HIP(hipMemcpyAsync(d_nshift, nshift.data(), (size_t)dz * sizeof(double), hipMemcpyHostToDevice, st));
    IVX_HIP(hipMemsetAsync(d_old, 0x7f, (size_t)dz * 2 * sizeof(int), st)); // 0x7f7f7f7f: above every sample
    const double zn1 = ig::pole_power(dy);
    const int64_t xb = ivx::cdiv(dx, 64);
    for (int64_t z0 = 0; z0 < dz; z0 += per) {
        const int64_t nz = std::min(per, dz - z0);
        int rc = launch1d(k_tilt_columns, nz * xb * 64, 64, st, "image_fix_gantry_tilt", vol, z0, nz, dy, dx, (const double *)d_nshift, zn1,
                          d_coef, d_old, d_new);
        if (rc) return rc;
    }
    std::vector<int> mins((size_t)dz * 2), cval((size_t)dz);
    IVX_HIP(hipMemcpyAsync(mins.data(), d_old, (size_t)dz * 2 * sizeof(int), hipMemcpyDeviceToHost, st));
    IVX_HIP(hipStreamSynchronize(st));
    std::vector<uint8_t> fills((size_t)dz);
    for (int64_t n = 0; n < dz; n++) fills[(size_t)n] = ig::has_fill_rows(dy, nshift[(size_t)n]);
    ig::resolve_cvals(dz, mins.data(), mins.data() + dz, fills.data(), cval.data());
    IVX_HIP(hipMemcpyAsync(d_cval, cval.data(), (size_t)dz * sizeof(int), hipMemcpyHostToDevice, st));
    IVX_HIP(hipStreamSynchronize(st)); // (cval goes out of scope)
    IVX_REQUIRE(dz * dy < ((int64_t)1 << 31), IVX_EINVAL, "image_fix_gantry_tilt: %lld rows", (long long)(dz * dy));
    hipLaunchKernelGGL(k_tilt_fill, dim3((unsigned)(dz * dy)), dim3(256), 0, st, vol, dz, dy, dx, (const double *)d_nshift, (const int *)d_cval);
    IVX_LAUNCH_CHECK();
    if (cvals_out) memcpy(cvals_out, cval.data(), (size_t)dz * sizeof(int));
    return IVX_OK;
}

// ---- host forms -----------------------------------------------------------------------------------------------------------------
extern "C" int ivx_image_flip(void *vol, const int64_t shape[3], const int64_t strides[3], size_t isz, int axis) {
    ivx::HostCallGuard host_guard__;
    using namespace ivx;
    IVX_REQUIRE(vol && shape && strides, IVX_EINVAL, "image_flip: null");
    if (!check_dims("image_flip", shape[0], shape[1], shape[2], isz)) return IVX_EINVAL;
    const size_t n = (size_t)shape[0] * shape[1] * shape[2] * isz;
    if (n == 0) return IVX_OK;
    void *d;
    int rc;
    if ((rc = ws_get(WS_OUT, n, &d))) return rc;
    if ((rc = upload_strided(d, vol, shape, strides, isz, WS_OUT))) return rc;
    if ((rc = ivx_dev_image_flip(d, shape[0], shape[1], shape[2], isz, axis, nullptr))) return rc;
    IVX_HIP(hipDeviceSynchronize());
    return download_strided(vol, shape, strides, d, isz, WS_OUT);
}

extern "C" int ivx_image_swap_axes(const void *src, const int64_t shape[3], const int64_t strides[3], size_t isz, int a, int b, void *dst,
                                   const int64_t dst_strides[3]) {
    ivx::HostCallGuard host_guard__;
    using namespace ivx;
    IVX_REQUIRE(src && dst && shape && strides && dst_strides, IVX_EINVAL, "image_swap_axes: null");
    IVX_REQUIRE(a >= 0 && a <= 2 && b >= 0 && b <= 2 && a != b, IVX_EINVAL, "image_swap_axes: axes (%d, %d)", a, b);
    if (!check_dims("image_swap_axes", shape[0], shape[1], shape[2], isz)) return IVX_EINVAL;
    const size_t n = (size_t)shape[0] * shape[1] * shape[2] * isz;
    if (n == 0) return IVX_OK;
    int64_t oshape[3] = {shape[0], shape[1], shape[2]};
    std::swap(oshape[a], oshape[b]);
    void *d_in, *d_out;
    int rc;
    if ((rc = ws_get(WS_IN, n, &d_in))) return rc;
    if ((rc = ws_get(WS_OUT, n, &d_out))) return rc;
    if ((rc = upload_strided(d_in, src, shape, strides, isz, WS_IN))) return rc;
    if ((rc = ivx_dev_image_swap_axes(d_in, shape[0], shape[1], shape[2], isz, a, b, d_out, nullptr))) return rc;
    IVX_HIP(hipDeviceSynchronize());
    return download_strided(dst, oshape, dst_strides, d_out, isz, WS_OUT);
}

extern "C" int ivx_image_fix_gantry_tilt(int16_t *vol, const int64_t shape[3], const int64_t strides[3], const double *shifts, int *cvals_out) {
    ivx::HostCallGuard host_guard__;
    using namespace ivx;
    IVX_REQUIRE(vol && shape && strides && shifts, IVX_EINVAL, "image_fix_gantry_tilt: null");
    if (!check_dims("image_fix_gantry_tilt", shape[0], shape[1], shape[2], 8)) return IVX_EINVAL;
    const size_t n = (size_t)shape[0] * shape[1] * shape[2] * 2;
    if (n == 0) return IVX_OK;
    size_t sb = 0;
    void *d, *d_s;
    int rc;
    if ((rc = ivx_image_tilt_scratch_bytes(shape[0], shape[1], shape[2], &sb))) return rc;
    if ((rc = ws_get(WS_OUT, n, &d))) return rc;
    if ((rc = ws_get(WS_AUX0, sb, &d_s))) return rc;
    if ((rc = upload_strided(d, vol, shape, strides, 2, WS_OUT))) return rc;
    if ((rc = ivx_dev_image_fix_gantry_tilt((int16_t *)d, shape[0], shape[1], shape[2], shifts, d_s, sb, cvals_out, nullptr))) return rc;
    IVX_HIP(hipDeviceSynchronize());
    return download_strided(vol, shape, strides, d, 2, WS_OUT);
}
