// k_filter.hip -- the Image Filters dialog on the GPU: Gaussian, median, mean, sharpen, despeckle, border detection.
//
// Replaces invesalius/data/filters.py:5-66 (scipy.ndimage gaussian_filter / median_filter / uniform_filter / sobel on the
// whole Slice.matrix) as dispatched by Slice.__apply_image_filter / _run_filter (invesalius/data/slice_.py:2330-2430),
// 3-D or slice by slice ("2D": the slice axis gets no pass and a window extent of 1).  scipy's arithmetic restated
// (ni_filters.c NI_Correlate1D / NI_UniformFilter1D / NI_RankFilter, ni_support.c NI_EXTEND_REFLECT), bit for bit:
//   * boundaries: mode "reflect" (d c b a | a b c d | d c b a), periodic in 2n, so radii >= the axis length fold again;
//   * symmetric correlate (Gaussian, the [1,2,1] of Sobel): y = x[0]*w[0]; y += (x[-j] + x[+j]) * w[j], j = r .. 1;
//     antisymmetric ([-1,0,1]): y = x[0]*0; y += (x[-1] - x[+1]) * -1.  One pass per axis in increasing axis order,
//     float64, the pass's output type in between (int16 -> truncated, C cast; float64 -> kept);
//   * box sum: the window sum is an exact integer, trunc(S / s) == C integer division for every int16 sum;
//   * median: element (s^d)//2 of the sorted window, offsets -(s//2) .. s-1-s//2 (the upper median for even s).
// The Gaussian weights come from the caller (numpy's exp; libm's may differ in the last bit and the int16 truncation
// turns that into a different voxel).  Everything is compiled with -ffp-contract=off: no FMA where scipy has none.
// Median: per output, the rank is found by a bitwise binary search over the value range [min, max] of the window held in
// registers -- #(v < t) per candidate bit, two VALU ops per window element and bit (see DESIGN.md "Image filters").
#include <math.h>

#include "ivx_internal.h"

namespace {
using namespace ivx;

struct FWeights { // w[0] centre, w[j] the weight of offsets -j and +j
    double w[IVX_FILTER_MAX_RADIUS + 1];
};

struct Dims {
    int nz, ny, nx;
};

__device__ __forceinline__ int refl(int i, int n) {
    if ((unsigned)i < (unsigned)n) return i;
    const int p = 2 * n;
    i %= p;
    if (i < 0) i += p;
    return i < n ? i : p - 1 - i;
}

__device__ __forceinline__ int16_t trunc16(double v) { return (int16_t)(int32_t)v; } // numpy astype(int16) on x86-64

template <typename T> __device__ __forceinline__ T cvt_out(double v);
template <> __device__ __forceinline__ int16_t cvt_out<int16_t>(double v) { return trunc16(v); }
template <> __device__ __forceinline__ double cvt_out<double>(double v) { return v; }

__device__ __forceinline__ int64_t ax_stride(Dims d, int ax) { return ax == 0 ? (int64_t)d.ny * d.nx : (ax == 1 ? d.nx : 1); }

// one symmetric correlate pass along `ax` straight from global memory (radii whose tile does not fit in LDS);
// block (64, 4), grid (cdiv(nx, 64), cdiv(ny, 4), nz)
template <typename Ti, typename To>
__global__ __launch_bounds__(256) void k_sym_pass(const Ti *__restrict__ in, To *__restrict__ out, Dims d, int ax, int r, FWeights W) {
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y, z = blockIdx.z;
    if (x >= d.nx || y >= d.ny) return;
    const int64_t i = ((int64_t)z * d.ny + y) * d.nx + x;
    const int c = ax == 0 ? z : (ax == 1 ? y : x), n = ax == 0 ? d.nz : (ax == 1 ? d.ny : d.nx);
    const int64_t st = ax_stride(d, ax);
    double acc = (double)in[i] * W.w[0];
    if (c - r >= 0 && c + r < n) {
        for (int j = r; j >= 1; j--) {
            const double s = (double)in[i - j * st] + (double)in[i + j * st];
            acc += s * W.w[j];
        }
    } else {
        const int64_t base = i - c * st;
        for (int j = r; j >= 1; j--) {
            const double s = (double)in[base + refl(c - j, n) * st] + (double)in[base + refl(c + j, n) * st];
            acc += s * W.w[j];
        }
    }
    out[i] = cvt_out<To>(acc);
}

// The same pass staged in LDS (one coalesced load of the tile and its reflected halo, then every tap from LDS), used
// whenever the tile fits in 64 KB.  Along x: a block owns XT outputs of one row.  Along z or y: a block owns 64 x-positions
// times LT outputs along the axis, lanes (64, 4).
constexpr int XT = 1024, LT = 64;

template <typename Ti, typename To>
__global__ __launch_bounds__(256) void k_sym_x(const Ti *__restrict__ in, To *__restrict__ out, Dims d, int r, FWeights W) {
    extern __shared__ __align__(16) unsigned char smem_raw[];
    Ti *s = reinterpret_cast<Ti *>(smem_raw);
    const int x0 = blockIdx.x * XT, y = blockIdx.y, z = blockIdx.z, tid = threadIdx.x;
    const int64_t row = ((int64_t)z * d.ny + y) * d.nx;
    const int ext = min(XT, d.nx - x0) + 2 * r;
    for (int e = tid; e < ext; e += 256) s[e] = in[row + refl(x0 - r + e, d.nx)];
    __syncthreads();
    for (int q = tid; q < XT; q += 256) {
        const int x = x0 + q;
        if (x >= d.nx) break;
        const Ti *c = s + q + r;
        double acc = (double)c[0] * W.w[0];
        for (int j = r; j >= 1; j--) {
            const double t = (double)c[-j] + (double)c[j];
            acc += t * W.w[j];
        }
        out[row + x] = cvt_out<To>(acc);
    }
}

template <typename Ti, typename To>
__global__ __launch_bounds__(256) void k_sym_zy(const Ti *__restrict__ in, To *__restrict__ out, Dims d, int ax, int r, FWeights W) {
    extern __shared__ __align__(16) unsigned char smem_raw[];
    Ti *s = reinterpret_cast<Ti *>(smem_raw);
    const int x0 = blockIdx.x * 64, o = blockIdx.y, c0 = blockIdx.z * LT, tx = threadIdx.x, ty = threadIdx.y;
    const int n = ax == 0 ? d.nz : d.ny;
    const int64_t st = ax == 0 ? (int64_t)d.ny * d.nx : d.nx;
    const int64_t base = (ax == 0 ? (int64_t)o * d.nx : (int64_t)o * d.ny * d.nx) + x0; // + c * st + xx
    const int nl = min(LT, n - c0) + 2 * r, nxb = min(64, d.nx - x0);
    for (int e = ty * 64 + tx; e < nl * 64; e += 256) {
        const int l = e >> 6, xx = e & 63;
        if (xx < nxb) s[e] = in[base + (int64_t)refl(c0 - r + l, n) * st + xx];
    }
    __syncthreads();
    if (tx >= nxb) return;
    for (int l = ty; l < LT; l += 4) {
        const int c = c0 + l;
        if (c >= n) break;
        const Ti *p = s + (l + r) * 64 + tx;
        double acc = (double)p[0] * W.w[0];
        for (int j = r; j >= 1; j--) {
            const double t = (double)p[-j * 64] + (double)p[j * 64];
            acc += t * W.w[j];
        }
        out[base + (int64_t)c * st + tx] = cvt_out<To>(acc);
    }
}

__global__ __launch_bounds__(256) void k_widen(const int16_t *__restrict__ in, double *__restrict__ out, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = (double)in[i];
}

// box pass along `ax`: one thread per run of `seg` outputs of a line, a sliding exact int32 window sum (cost independent
// of the size).  Threads enumerate (segment, line) with x fastest for ax 0 / 1 (coalesced), rows for ax 2.
__global__ __launch_bounds__(256) void k_box_pass(const int16_t *__restrict__ in, int16_t *__restrict__ out, Dims d, int ax, int s,
                                                  int seg, int64_t nlines, int nseg) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= nlines * nseg) return;
    int64_t l;
    int sg;
    if (ax == 2) { l = t / nseg; sg = (int)(t % nseg); }
    else { sg = (int)(t / nlines); l = t % nlines; }
    int64_t base, st;
    int n;
    if (ax == 0) { base = l; st = (int64_t)d.ny * d.nx; n = d.nz; }
    else if (ax == 1) { const int64_t zz = l / d.nx, xx = l % d.nx; base = zz * d.ny * d.nx + xx; st = d.nx; n = d.ny; }
    else { base = l * d.nx; st = 1; n = d.nx; }
    const int c0 = sg * seg, c1 = min(c0 + seg, n), lo = s / 2;
    int32_t sum = 0;
    for (int k = c0 - lo; k < c0 - lo + s; k++) sum += in[base + (int64_t)refl(k, n) * st];
    out[base + (int64_t)c0 * st] = (int16_t)(sum / s);
    for (int c = c0 + 1; c < c1; c++) {
        sum += (int32_t)in[base + (int64_t)refl(c - lo + s - 1, n) * st] - (int32_t)in[base + (int64_t)refl(c - lo - 1, n) * st];
        out[base + (int64_t)c * st] = (int16_t)(sum / s);
    }
}

// -- median ------------------------------------------------------------------------------------------------------------
// The rank-th smallest of v[0..N): lo = min; for each bit b of (max - min) from the top, t = lo + 2^b replaces lo when
// #(v < t) <= rank.  Invariant: #(v < lo) <= rank < #(v < lo + 2^(b+1)); after bit 0 lo is the answer.
template <int N>
__device__ __forceinline__ int select_rank(const int (&v)[N], int rank) {
    int mn = v[0], mx = v[0];
#pragma unroll
    for (int i = 1; i < N; i++) {
        mn = min(mn, v[i]);
        mx = max(mx, v[i]);
    }
    if (mn == mx) return mn;
    int lo = mn;
    for (int b = 31 - __clz((unsigned)(mx - mn)); b >= 0; b--) {
        const int t = lo + (1 << b);
        int cnt = 0;
#pragma unroll
        for (int i = 0; i < N; i++) cnt += v[i] < t ? 1 : 0;
        if (cnt <= rank) lo = t;
    }
    return lo;
}

constexpr int MTX = 32, MTY = 8, MTZ = 4; // output tile of one block of 256 threads (x, y), looping over MTZ slices

template <int WZ, int WY, int WX>
__global__ __launch_bounds__(256) void k_median(const int16_t *__restrict__ in, int16_t *__restrict__ out, Dims d) {
    constexpr int LZ = MTZ + WZ - 1, LY = MTY + WY - 1, LX = MTX + WX - 1, N = WZ * WY * WX;
    __shared__ int16_t tile[LZ * LY * LX];
    const int x0 = blockIdx.x * MTX, y0 = blockIdx.y * MTY, z0 = blockIdx.z * MTZ;
    const int tid = threadIdx.y * MTX + threadIdx.x;
    for (int e = tid; e < LZ * LY * LX; e += 256) {
        const int lx = e % LX, ly = (e / LX) % LY, lz = e / (LX * LY);
        const int gz = refl(z0 - WZ / 2 + lz, d.nz), gy = refl(y0 - WY / 2 + ly, d.ny), gx = refl(x0 - WX / 2 + lx, d.nx);
        tile[e] = in[((int64_t)gz * d.ny + gy) * d.nx + gx];
    }
    __syncthreads();
    const int x = x0 + threadIdx.x, y = y0 + threadIdx.y;
    if (x >= d.nx || y >= d.ny) return;
    for (int tz = 0; tz < MTZ; tz++) {
        const int z = z0 + tz;
        if (z >= d.nz) break;
        int v[N];
#pragma unroll
        for (int a = 0; a < WZ; a++)
#pragma unroll
            for (int b = 0; b < WY; b++)
#pragma unroll
                for (int c = 0; c < WX; c++) v[(a * WY + b) * WX + c] = tile[((tz + a) * LY + threadIdx.y + b) * LX + threadIdx.x + c];
        out[((int64_t)z * d.ny + y) * d.nx + x] = (int16_t)select_rank<N>(v, N / 2);
    }
}

// -- Sobel magnitude ---------------------------------------------------------------------------------------------------
__device__ __forceinline__ double sob_d(double m, double c, double p) { // correlate1d [-1, 0, 1], antisymmetric path
    double y = c * 0.0;
    y += (m - p) * -1.0;
    return y;
}
__device__ __forceinline__ double sob_s(double m, double c, double p) { // correlate1d [1, 2, 1], symmetric path
    double y = c * 2.0;
    y += (m + p) * 1.0;
    return y;
}

constexpr int STX = 32, STY = 8, STZ = 4;

// P = plane axis (-1: 3-D).  G[a][b][c] is the 3^3 neighbourhood (index 1 only along P); sobel(axis k) correlates along k,
// then along every other (non-plane) axis in increasing order; M = sqrt of the sum of squares in increasing axis order.
template <int P>
__global__ __launch_bounds__(256) void k_sobel_mag(const double *__restrict__ g, double *__restrict__ mag, Dims d) {
    constexpr int HZ = P == 0 ? 0 : 1, HY = P == 1 ? 0 : 1, HX = P == 2 ? 0 : 1;
    constexpr int LZ = STZ + 2 * HZ, LY = STY + 2 * HY, LX = STX + 2 * HX;
    __shared__ double tile[LZ * LY * LX];
    const int x0 = blockIdx.x * STX, y0 = blockIdx.y * STY, z0 = blockIdx.z * STZ;
    const int tid = threadIdx.y * STX + threadIdx.x;
    for (int e = tid; e < LZ * LY * LX; e += 256) {
        const int lx = e % LX, ly = (e / LX) % LY, lz = e / (LX * LY);
        const int gz = refl(z0 - HZ + lz, d.nz), gy = refl(y0 - HY + ly, d.ny), gx = refl(x0 - HX + lx, d.nx);
        tile[e] = g[((int64_t)gz * d.ny + gy) * d.nx + gx];
    }
    __syncthreads();
    const int x = x0 + threadIdx.x, y = y0 + threadIdx.y;
    if (x >= d.nx || y >= d.ny) return;
    for (int tz = 0; tz < STZ; tz++) {
        const int z = z0 + tz;
        if (z >= d.nz) break;
        double G[3][3][3];
#pragma unroll
        for (int a = 0; a < 3; a++)
#pragma unroll
            for (int b = 0; b < 3; b++)
#pragma unroll
                for (int c = 0; c < 3; c++) {
                    const int la = HZ ? a : 0, lb = HY ? b : 0, lc = HX ? c : 0;
                    G[a][b][c] = tile[((tz + la) * LY + threadIdx.y + lb) * LX + threadIdx.x + lc];
                }
        double m;
        if (P < 0) {
            double A[3][3], B[3], s0, s1, s2;
            // axis 0, then 1, then 2
            for (int b = 0; b < 3; b++)
                for (int c = 0; c < 3; c++) A[b][c] = sob_d(G[0][b][c], G[1][b][c], G[2][b][c]);
            for (int c = 0; c < 3; c++) B[c] = sob_s(A[0][c], A[1][c], A[2][c]);
            s0 = sob_s(B[0], B[1], B[2]);
            // axis 1, then 0, then 2
            for (int a = 0; a < 3; a++)
                for (int c = 0; c < 3; c++) A[a][c] = sob_d(G[a][0][c], G[a][1][c], G[a][2][c]);
            for (int c = 0; c < 3; c++) B[c] = sob_s(A[0][c], A[1][c], A[2][c]);
            s1 = sob_s(B[0], B[1], B[2]);
            // axis 2, then 0, then 1
            for (int a = 0; a < 3; a++)
                for (int b = 0; b < 3; b++) A[a][b] = sob_d(G[a][b][0], G[a][b][1], G[a][b][2]);
            for (int b = 0; b < 3; b++) B[b] = sob_s(A[0][b], A[1][b], A[2][b]);
            s2 = sob_s(B[0], B[1], B[2]);
            double q = s0 * s0;
            q += s1 * s1;
            q += s2 * s2;
            m = __dsqrt_rn(q);
        } else {
            double A[3], s0, s1;
            if (P == 0) { // axes 1, 2
                for (int c = 0; c < 3; c++) A[c] = sob_d(G[1][0][c], G[1][1][c], G[1][2][c]);
                s0 = sob_s(A[0], A[1], A[2]);
                for (int b = 0; b < 3; b++) A[b] = sob_d(G[1][b][0], G[1][b][1], G[1][b][2]);
                s1 = sob_s(A[0], A[1], A[2]);
            } else if (P == 1) { // axes 0, 2
                for (int c = 0; c < 3; c++) A[c] = sob_d(G[0][1][c], G[1][1][c], G[2][1][c]);
                s0 = sob_s(A[0], A[1], A[2]);
                for (int a = 0; a < 3; a++) A[a] = sob_d(G[a][1][0], G[a][1][1], G[a][1][2]);
                s1 = sob_s(A[0], A[1], A[2]);
            } else { // axes 0, 1
                for (int b = 0; b < 3; b++) A[b] = sob_d(G[0][b][1], G[1][b][1], G[2][b][1]);
                s0 = sob_s(A[0], A[1], A[2]);
                for (int a = 0; a < 3; a++) A[a] = sob_d(G[a][0][1], G[a][1][1], G[a][2][1]);
                s1 = sob_s(A[0], A[1], A[2]);
            }
            double q = s0 * s0;
            q += s1 * s1;
            m = __dsqrt_rn(q);
        }
        mag[((int64_t)z * d.ny + y) * d.nx + x] = m;
    }
}

// -- per-segment (whole volume or per slice) min / max -------------------------------------------------------------------
// int16 -> int keys; non-negative float64 (magnitudes) -> their bit patterns, ordered like the values.
__device__ __forceinline__ int key_of(int16_t v) { return v; }
__device__ __forceinline__ unsigned long long key_of(double v) { return (unsigned long long)__double_as_longlong(v); }

template <typename K>
__global__ void k_seg_init(K *mn, K *mx, int nseg, K hi, K lo) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < nseg) {
        mn[i] = hi;
        mx[i] = lo;
    }
}

template <typename K>
__device__ void block_minmax_commit(K lmn, K lmx, K *mn, K *mx) {
    __shared__ K smn[256], smx[256];
    const int tid = threadIdx.y * blockDim.x + threadIdx.x;
    smn[tid] = lmn;
    smx[tid] = lmx;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if (tid < h) {
            smn[tid] = min(smn[tid], smn[tid + h]);
            smx[tid] = max(smx[tid], smx[tid + h]);
        }
        __syncthreads();
    }
    if (tid == 0) {
        atomicMin(mn, smn[0]);
        atomicMax(mx, smx[0]);
    }
}

// segments constant along rows (P = -1, 0, 1): grid (row chunks, nseg), 256 threads stride over the rows of the chunk
template <typename T, typename K>
__global__ __launch_bounds__(256) void k_seg_minmax_rows(const T *__restrict__ in, Dims d, int P, int rpb, K *mn, K *mx, K hi, K lo) {
    const int sgi = blockIdx.y;
    int64_t rows, base, rst;
    if (P < 0) { rows = (int64_t)d.nz * d.ny; base = 0; rst = d.nx; }
    else if (P == 0) { rows = d.ny; base = (int64_t)sgi * d.ny * d.nx; rst = d.nx; }
    else { rows = d.nz; base = (int64_t)sgi * d.nx; rst = (int64_t)d.ny * d.nx; }
    const int64_t r0 = (int64_t)blockIdx.x * rpb, r1 = min(r0 + rpb, rows);
    K lmn = hi, lmx = lo;
    for (int64_t r = r0; r < r1; r++) {
        const T *row = in + base + r * rst;
        for (int x = threadIdx.x; x < d.nx; x += 256) {
            const K k = key_of(row[x]);
            lmn = min(lmn, k);
            lmx = max(lmx, k);
        }
    }
    if (r0 >= rows) return; // uniform per block
    block_minmax_commit<K>(lmn, lmx, mn + sgi, mx + sgi);
}

// segments along x (P = 2): block (64 x, 4 rows), grid (cdiv(nx, 64), row chunks); reduce over the 4 row lanes per x
template <typename T, typename K>
__global__ __launch_bounds__(256) void k_seg_minmax_x(const T *__restrict__ in, Dims d, int rpb, K *mn, K *mx, K hi, K lo) {
    __shared__ K smn[4][64], smx[4][64];
    const int x = blockIdx.x * 64 + threadIdx.x;
    const int64_t rows = (int64_t)d.nz * d.ny, r0 = (int64_t)blockIdx.y * rpb, r1 = min(r0 + rpb, rows);
    K lmn = hi, lmx = lo;
    if (x < d.nx)
        for (int64_t r = r0 + threadIdx.y; r < r1; r += 4) {
            const K k = key_of(in[r * d.nx + x]);
            lmn = min(lmn, k);
            lmx = max(lmx, k);
        }
    smn[threadIdx.y][threadIdx.x] = lmn;
    smx[threadIdx.y][threadIdx.x] = lmx;
    __syncthreads();
    if (threadIdx.y == 0 && x < d.nx && r0 < rows) {
        for (int q = 1; q < 4; q++) {
            lmn = min(lmn, smn[q][threadIdx.x]);
            lmx = max(lmx, smx[q][threadIdx.x]);
        }
        atomicMin(mn + x, lmn);
        atomicMax(mx + x, lmx);
    }
}

__device__ __forceinline__ int seg_of(int64_t i, Dims d, int P) {
    if (P < 0) return 0;
    if (P == 0) return (int)(i / ((int64_t)d.ny * d.nx));
    if (P == 1) return (int)((i / d.nx) % d.ny);
    return (int)(i % d.nx);
}

// sharpen: f + a (f - b), clipped to the segment's [min, max], truncated
__global__ __launch_bounds__(256) void k_sharpen_final(const int16_t *__restrict__ m, const double *__restrict__ b, int16_t *__restrict__ out,
                                                       Dims d, int P, const int *__restrict__ mn, const int *__restrict__ mx, double a) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x, n = (int64_t)d.nz * d.ny * d.nx;
    if (i >= n) return;
    const int sg = seg_of(i, d, P);
    const double f = (double)m[i];
    const double det = f - b[i];
    double v = f + a * det;
    const double lo = (double)mn[sg], hi = (double)mx[sg];
    v = v < lo ? lo : v; // np.clip: maximum(v, lo), then minimum(., hi)
    v = v > hi ? hi : v;
    out[i] = trunc16(v);
}

// border detection: ((M - Mmin) / (Mmax - Mmin)) * (max - min) + min when normalising over a non-flat segment, else M
__global__ __launch_bounds__(256) void k_border_final(const double *__restrict__ M, int16_t *__restrict__ out, Dims d, int P,
                                                      const unsigned long long *__restrict__ Mmn, const unsigned long long *__restrict__ Mmx,
                                                      const int *__restrict__ mn, const int *__restrict__ mx, int normalize) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x, n = (int64_t)d.nz * d.ny * d.nx;
    if (i >= n) return;
    double v = M[i];
    if (normalize) {
        const int sg = seg_of(i, d, P);
        const double mlo = __longlong_as_double((long long)Mmn[sg]), mhi = __longlong_as_double((long long)Mmx[sg]);
        const double range = mhi - mlo;
        if (range > 0) {
            const double lo = (double)mn[sg], hi = (double)mx[sg];
            const double span = hi - lo;
            double t = v - mlo;
            t = t / range;
            t = t * span;
            v = t + lo;
        }
    }
    out[i] = trunc16(v);
}

// -- host-side plumbing ------------------------------------------------------------------------------------------------
struct Geo {
    Dims d;
    int64_t n;
    int P, nseg;
    int axes[3], naxes; // the pass axes in increasing order (all but P)
};

static int make_geo(const int64_t shape[3], int plane_axis, Geo &g) {
    IVX_REQUIRE(shape, IVX_EINVAL, "filter: null shape");
    for (int a = 0; a < 3; a++)
        IVX_REQUIRE(shape[a] > 0 && shape[a] < 65536, IVX_EINVAL, "filter: shape[%d] = %lld out of range", a, (long long)shape[a]);
    IVX_REQUIRE(plane_axis >= -1 && plane_axis <= 2, IVX_EINVAL, "filter: plane_axis %d (-1 = 3-D, 0/1/2 = slices)", plane_axis);
    g.d = {(int)shape[0], (int)shape[1], (int)shape[2]};
    g.n = shape[0] * shape[1] * shape[2];
    g.P = plane_axis;
    g.nseg = plane_axis < 0 ? 1 : (int)shape[plane_axis];
    g.naxes = 0;
    for (int a = 0; a < 3; a++)
        if (a != plane_axis) g.axes[g.naxes++] = a;
    return IVX_OK;
}

static inline size_t al(size_t b) { return (b + 255) & ~(size_t)255; }

static int load_weights(const double *w, int radius, FWeights &W) {
    IVX_REQUIRE(radius <= IVX_FILTER_MAX_RADIUS, IVX_EINVAL, "filter: radius %d > %d", radius, IVX_FILTER_MAX_RADIUS);
    memset(&W, 0, sizeof(W));
    if (radius < 0) return IVX_OK;
    IVX_REQUIRE(w, IVX_EINVAL, "filter: null weights");
    // w holds the 2r+1 weights of scipy's kernel (symmetric); the centre and the +j side are what the symmetric path uses
    for (int j = 0; j <= radius; j++) W.w[j] = w[radius + j];
    return IVX_OK;
}

template <typename Ti, typename To>
static int sym_pass(const Ti *in, To *out, const Geo &g, int ax, int r, const FWeights &W, hipStream_t st) {
    if (ax == 2 && (size_t)(XT + 2 * r) * sizeof(Ti) <= 65536) {
        dim3 grid((unsigned)cdiv(g.d.nx, XT), (unsigned)g.d.ny, (unsigned)g.d.nz);
        hipLaunchKernelGGL((k_sym_x<Ti, To>), grid, dim3(256), (XT + 2 * r) * sizeof(Ti), st, in, out, g.d, r, W);
        IVX_LAUNCH_CHECK();
        return IVX_OK;
    }
    if (ax != 2 && (size_t)(LT + 2 * r) * 64 * sizeof(Ti) <= 65536) {
        dim3 grid((unsigned)cdiv(g.d.nx, 64), (unsigned)(ax == 0 ? g.d.ny : g.d.nz), (unsigned)cdiv(ax == 0 ? g.d.nz : g.d.ny, LT));
        hipLaunchKernelGGL((k_sym_zy<Ti, To>), grid, dim3(64, 4), (LT + 2 * r) * 64 * sizeof(Ti), st, in, out, g.d, ax, r, W);
        IVX_LAUNCH_CHECK();
        return IVX_OK;
    }
    dim3 grid((unsigned)cdiv(g.d.nx, 64), (unsigned)cdiv(g.d.ny, 4), (unsigned)g.d.nz);
    hipLaunchKernelGGL((k_sym_pass<Ti, To>), grid, dim3(64, 4), 0, st, in, out, g.d, ax, r, W);
    IVX_LAUNCH_CHECK();
    return IVX_OK;
}

// float64 Gaussian of int16 `in` (no truncation between passes) into f0 / f1; *res = the buffer holding it
static int gauss_f64(const int16_t *in, const Geo &g, const FWeights &W, int r, double *f0, double *f1, double **res, hipStream_t st) {
    int rc;
    if (r < 0) { // sigma <= 1e-15 on every axis: scipy copies
        hipLaunchKernelGGL(k_widen, dim3((unsigned)cdiv(g.n, 256)), dim3(256), 0, st, in, f0, g.n);
        IVX_LAUNCH_CHECK();
        *res = f0;
        return IVX_OK;
    }
    double *bufs[2] = {f0, f1};
    for (int k = 0; k < g.naxes; k++) {
        double *dst = bufs[k & 1];
        if (k == 0) rc = sym_pass<int16_t, double>(in, dst, g, g.axes[k], r, W, st);
        else rc = sym_pass<double, double>(bufs[(k - 1) & 1], dst, g, g.axes[k], r, W, st);
        if (rc) return rc;
        *res = dst;
    }
    return IVX_OK;
}

template <typename T, typename K>
static int seg_minmax(const T *in, const Geo &g, K *mn, K *mx, K hi, K lo, hipStream_t st) {
    hipLaunchKernelGGL((k_seg_init<K>), dim3((unsigned)cdiv(g.nseg, 256)), dim3(256), 0, st, mn, mx, g.nseg, hi, lo);
    IVX_LAUNCH_CHECK();
    const int rpb = (int)std::max<int64_t>(1, 8192 / g.d.nx);
    if (g.P == 2) {
        const int64_t rows = (int64_t)g.d.nz * g.d.ny, rp = std::max<int64_t>(rpb, 64);
        dim3 grid((unsigned)cdiv(g.d.nx, 64), (unsigned)cdiv(rows, rp));
        hipLaunchKernelGGL((k_seg_minmax_x<T, K>), grid, dim3(64, 4), 0, st, in, g.d, (int)rp, mn, mx, hi, lo);
    } else {
        const int64_t rows = g.P < 0 ? (int64_t)g.d.nz * g.d.ny : (g.P == 0 ? g.d.ny : g.d.nz);
        dim3 grid((unsigned)cdiv(rows, rpb), (unsigned)g.nseg);
        hipLaunchKernelGGL((k_seg_minmax_rows<T, K>), grid, dim3(256), 0, st, in, g.d, g.P, rpb, mn, mx, hi, lo);
    }
    IVX_LAUNCH_CHECK();
    return IVX_OK;
}

struct FScratch {
    double *f0, *f1;
    int *mn, *mx;
    unsigned long long *Mmn, *Mmx;
};

static void carve(void *scratch, const Geo &g, FScratch &s) {
    char *p = (char *)scratch;
    const size_t fv = al((size_t)g.n * 8), sv = al((size_t)g.nseg * 8);
    s.f0 = (double *)p;
    s.f1 = (double *)(p + fv);
    s.mn = (int *)(p + 2 * fv);
    s.mx = (int *)(p + 2 * fv + sv);
    s.Mmn = (unsigned long long *)(p + 2 * fv + 2 * sv);
    s.Mmx = (unsigned long long *)(p + 2 * fv + 3 * sv);
}

static int check_io(const int16_t *in, const int16_t *out, const void *scratch, bool need_scratch) {
    IVX_REQUIRE(in && out, IVX_EINVAL, "filter: null buffer");
    IVX_REQUIRE(in != out, IVX_EINVAL, "filter: out must not alias in");
    IVX_REQUIRE(scratch || !need_scratch, IVX_EINVAL, "filter: null scratch");
    return IVX_OK;
}

static int median_size(double value, int *size) { // filters.py:11: max(3, min(int(2 * value + 1), 5))
    const double s = 2 * value + 1;
    IVX_REQUIRE(s == s, IVX_EINVAL, "filter: median value is NaN");
    *size = s >= 5 ? 5 : (s < 3 ? 3 : (int)s);
    return IVX_OK;
}

static int mean_size(double value, int *size) { // filters.py:17: int(2 * value + 1)
    const double s = 2 * value + 1;
    IVX_REQUIRE(s == s && s < 4096 && s > -4096, IVX_EINVAL, "filter: mean size int(2 * %g + 1) out of range", value);
    *size = (int)s;
    return IVX_OK;
}
} // namespace

extern "C" int ivx_filter_scratch_bytes(int kind, const int64_t shape[3], int plane_axis, size_t *nbytes) {
    Geo g;
    int rc = make_geo(shape, plane_axis, g);
    if (rc) return rc;
    IVX_REQUIRE(nbytes, IVX_EINVAL, "filter: null nbytes");
    switch (kind) {
    case IVX_FILTER_GAUSSIAN:
    case IVX_FILTER_DESPECKLE:
    case IVX_FILTER_MEAN: *nbytes = 2 * al((size_t)g.n * 2); break;
    case IVX_FILTER_MEDIAN: *nbytes = 0; break;
    case IVX_FILTER_SHARPEN:
    case IVX_FILTER_BORDER: *nbytes = 2 * al((size_t)g.n * 8) + 4 * al((size_t)g.nseg * 8); break;
    default: IVX_REQUIRE(false, IVX_EINVAL, "filter: unknown filter type %d", kind);
    }
    return IVX_OK;
}

extern "C" int ivx_dev_filter_gaussian_i16(const int16_t *in, const int64_t shape[3], int plane_axis, const double *w, int radius,
                                           int16_t *out, void *scratch, void *stream) {
    Geo g;
    FWeights W;
    int rc;
    if ((rc = make_geo(shape, plane_axis, g)) || (rc = check_io(in, out, scratch, true)) || (rc = load_weights(w, radius, W))) return rc;
    hipStream_t st = S(stream);
    if (radius < 0) {
        IVX_HIP(hipMemcpyAsync(out, in, (size_t)g.n * 2, hipMemcpyDeviceToDevice, st));
        return IVX_OK;
    }
    int16_t *bufs[2] = {(int16_t *)scratch, (int16_t *)((char *)scratch + al((size_t)g.n * 2))};
    for (int k = 0; k < g.naxes; k++) {
        const int16_t *src = k == 0 ? in : bufs[(k - 1) & 1];
        int16_t *dst = k == g.naxes - 1 ? out : bufs[k & 1];
        if ((rc = sym_pass<int16_t, int16_t>(src, dst, g, g.axes[k], radius, W, st))) return rc;
    }
    return IVX_OK;
}

extern "C" int ivx_dev_filter_median_i16(const int16_t *in, const int64_t shape[3], int plane_axis, int size, int16_t *out,
                                         void *stream) {
    Geo g;
    int rc;
    if ((rc = make_geo(shape, plane_axis, g)) || (rc = check_io(in, out, nullptr, false))) return rc;
    IVX_REQUIRE(size >= 3 && size <= 5, IVX_EINVAL, "filter: median size %d (3, 4 or 5)", size);
    dim3 grid((unsigned)cdiv(g.d.nx, MTX), (unsigned)cdiv(g.d.ny, MTY), (unsigned)cdiv(g.d.nz, MTZ));
    hipStream_t st = S(stream);
#define IVX_MED(WZ, WY, WX) hipLaunchKernelGGL((k_median<WZ, WY, WX>), grid, dim3(MTX, MTY), 0, st, in, out, g.d)
#define IVX_MED_P(S_)                                                                                                    \
    do {                                                                                                                 \
        if (plane_axis < 0) IVX_MED(S_, S_, S_);                                                                         \
        else if (plane_axis == 0) IVX_MED(1, S_, S_);                                                                    \
        else if (plane_axis == 1) IVX_MED(S_, 1, S_);                                                                    \
        else IVX_MED(S_, S_, 1);                                                                                         \
    } while (0)
    if (size == 3) IVX_MED_P(3);
    else if (size == 4) IVX_MED_P(4);
    else IVX_MED_P(5);
#undef IVX_MED_P
#undef IVX_MED
    IVX_LAUNCH_CHECK();
    return IVX_OK;
}

extern "C" int ivx_dev_filter_mean_i16(const int16_t *in, const int64_t shape[3], int plane_axis, int size, int16_t *out,
                                       void *scratch, void *stream) {
    Geo g;
    int rc;
    if ((rc = make_geo(shape, plane_axis, g)) || (rc = check_io(in, out, scratch, true))) return rc;
    IVX_REQUIRE(size < 4096, IVX_EINVAL, "filter: mean size %d", size);
    hipStream_t st = S(stream);
    if (size <= 1) { // scipy passes only the axes whose size is > 1
        IVX_HIP(hipMemcpyAsync(out, in, (size_t)g.n * 2, hipMemcpyDeviceToDevice, st));
        return IVX_OK;
    }
    int16_t *bufs[2] = {(int16_t *)scratch, (int16_t *)((char *)scratch + al((size_t)g.n * 2))};
    for (int k = 0; k < g.naxes; k++) {
        const int16_t *src = k == 0 ? in : bufs[(k - 1) & 1];
        int16_t *dst = k == g.naxes - 1 ? out : bufs[k & 1];
        const int ax = g.axes[k], n = ax == 0 ? g.d.nz : (ax == 1 ? g.d.ny : g.d.nx);
        const int seg = ax == 2 ? 16 : 64, nseg = (int)cdiv(n, seg);
        const int64_t nlines = g.n / n;
        hipLaunchKernelGGL(k_box_pass, dim3((unsigned)cdiv(nlines * nseg, 256)), dim3(256), 0, st, src, dst, g.d, ax, size, seg, nlines, nseg);
        IVX_LAUNCH_CHECK();
    }
    return IVX_OK;
}

extern "C" int ivx_dev_filter_sharpen_i16(const int16_t *in, const int64_t shape[3], int plane_axis, double value, const double *w,
                                          int radius, int16_t *out, void *scratch, void *stream) {
    Geo g;
    FWeights W;
    int rc;
    if ((rc = make_geo(shape, plane_axis, g)) || (rc = check_io(in, out, scratch, true)) || (rc = load_weights(w, radius, W))) return rc;
    hipStream_t st = S(stream);
    FScratch s;
    carve(scratch, g, s);
    double *b = nullptr;
    if ((rc = gauss_f64(in, g, W, radius, s.f0, s.f1, &b, st))) return rc;
    if ((rc = seg_minmax<int16_t, int>(in, g, s.mn, s.mx, 0x7fffffff, (int)0x80000000, st))) return rc;
    const double a = value * 0.5; // filters.py:29 `value * 0.5 * detail`
    hipLaunchKernelGGL(k_sharpen_final, dim3((unsigned)cdiv(g.n, 256)), dim3(256), 0, st, in, b, out, g.d, g.P, s.mn, s.mx, a);
    IVX_LAUNCH_CHECK();
    return IVX_OK;
}

extern "C" int ivx_dev_filter_border_i16(const int16_t *in, const int64_t shape[3], int plane_axis, int normalize, const double *w,
                                         int radius, int16_t *out, void *scratch, void *stream) {
    Geo g;
    FWeights W;
    int rc;
    if ((rc = make_geo(shape, plane_axis, g)) || (rc = check_io(in, out, scratch, true)) || (rc = load_weights(w, radius, W))) return rc;
    hipStream_t st = S(stream);
    FScratch s;
    carve(scratch, g, s);
    double *sm = nullptr;
    if ((rc = gauss_f64(in, g, W, radius, s.f0, s.f1, &sm, st))) return rc;
    double *mag = sm == s.f0 ? s.f1 : s.f0;
    dim3 grid((unsigned)cdiv(g.d.nx, STX), (unsigned)cdiv(g.d.ny, STY), (unsigned)cdiv(g.d.nz, STZ));
    if (plane_axis < 0) hipLaunchKernelGGL(k_sobel_mag<-1>, grid, dim3(STX, STY), 0, st, sm, mag, g.d);
    else if (plane_axis == 0) hipLaunchKernelGGL(k_sobel_mag<0>, grid, dim3(STX, STY), 0, st, sm, mag, g.d);
    else if (plane_axis == 1) hipLaunchKernelGGL(k_sobel_mag<1>, grid, dim3(STX, STY), 0, st, sm, mag, g.d);
    else hipLaunchKernelGGL(k_sobel_mag<2>, grid, dim3(STX, STY), 0, st, sm, mag, g.d);
    IVX_LAUNCH_CHECK();
    if (normalize) {
        if ((rc = seg_minmax<int16_t, int>(in, g, s.mn, s.mx, 0x7fffffff, (int)0x80000000, st))) return rc;
        if ((rc = seg_minmax<double, unsigned long long>(mag, g, s.Mmn, s.Mmx, ~0ull, 0ull, st))) return rc;
    }
    hipLaunchKernelGGL(k_border_final, dim3((unsigned)cdiv(g.n, 256)), dim3(256), 0, st, mag, out, g.d, g.P, s.Mmn, s.Mmx, s.mn, s.mx,
                       normalize ? 1 : 0);
    IVX_LAUNCH_CHECK();
    return IVX_OK;
}

extern "C" int ivx_image_filter(int kind, double value, int plane_axis, int normalize, const double *w, int radius, int dtype,
                                const void *img, const int64_t shape[3], const int64_t strides[3], void *out,
                                const int64_t ostrides[3]) {
    HostCallGuard guard;
    IVX_REQUIRE(dtype == IVX_I16, IVX_EINVAL, "filter: int16 images only (dtype code %d)", dtype);
    IVX_REQUIRE(img && out && strides && ostrides, IVX_EINVAL, "filter: null buffer");
    Geo g;
    int rc;
    if ((rc = make_geo(shape, plane_axis, g))) return rc;
    int size = 0;
    if (kind == IVX_FILTER_MEAN && (rc = mean_size(value, &size))) return rc;
    if (kind == IVX_FILTER_MEDIAN && (rc = median_size(value, &size))) return rc;
    size_t sb = 0;
    if ((rc = ivx_filter_scratch_bytes(kind, shape, plane_axis, &sb))) return rc;
    void *d_in = nullptr, *d_out = nullptr, *d_s = nullptr;
    if ((rc = ws_get(WS_IN, (size_t)g.n * 2, &d_in)) || (rc = ws_get(WS_OUT, (size_t)g.n * 2, &d_out)) || (rc = ws_get(WS_AUX0, sb, &d_s)))
        return rc;
    if ((rc = upload_strided(d_in, img, shape, strides, 2, WS_IN))) return rc;
    const int16_t *i16 = (const int16_t *)d_in;
    int16_t *o16 = (int16_t *)d_out;
    switch (kind) {
    case IVX_FILTER_GAUSSIAN:
    case IVX_FILTER_DESPECKLE: rc = ivx_dev_filter_gaussian_i16(i16, shape, plane_axis, w, radius, o16, d_s, nullptr); break;
    case IVX_FILTER_MEDIAN: rc = ivx_dev_filter_median_i16(i16, shape, plane_axis, size, o16, nullptr); break;
    case IVX_FILTER_MEAN: rc = ivx_dev_filter_mean_i16(i16, shape, plane_axis, size, o16, d_s, nullptr); break;
    case IVX_FILTER_SHARPEN: rc = ivx_dev_filter_sharpen_i16(i16, shape, plane_axis, value, w, radius, o16, d_s, nullptr); break;
    case IVX_FILTER_BORDER: rc = ivx_dev_filter_border_i16(i16, shape, plane_axis, normalize, w, radius, o16, d_s, nullptr); break;
    default: IVX_REQUIRE(false, IVX_EINVAL, "filter: unknown filter type %d", kind);
    }
    if (rc) return rc;
    IVX_HIP(hipDeviceSynchronize());
    return download_strided(out, shape, ostrides, d_out, 2, WS_OUT);
}
